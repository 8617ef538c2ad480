// tiff_write_kernels.h -- writing TIFF files with Deflate compression (zmi_tiff_write_dev; every byte of the file: include/zmi355.h,
// DESIGN.md section 25); included by pack.hip behind png_kernels.h and tiff_kernels.h.
//
// A page's segments -- strips or tiles -- run through the forward predictor into context scratch, are cut into pieces of piece_bytes
// and join ONE piece table that the independent-piece encoder works through in launch groups, exactly as the scanlines of
// zmi_png_encode_dev do: the payload copies are zmi_zip_pack_kernel, the places are pw_then's scan with a tail of 4 bytes.  The page's
// geometry is the caller's, so the plan (zmi_tw_plan, zmi_kernels.h) is worked out on the host and every kernel takes it by value;
// only the compressed sizes are device values.  The kernels:
//   zmi_tiff_wpieces_kernel   the piece table: piece i belongs to segment i / ppf, all segments but the last strip being alike
//   zmi_tiff_predict_kernel   the hot path, below
//   zmi_tiff_place_kernel     one group's places: zmi_png_place_kernel with the tail as a parameter
//   zmi_tiff_wmeta_kernel     header, IFD and the out-of-line values the host made from *w
//   zmi_tiff_wsegs_kernel     one wave per segment: the zero gap in front, the zlib header, the Adler-32, its offset and byte count in the
//                             file's two arrays, its words
//   zmi_tiff_wclose_kernel    the file's words and d_written
#pragma once

#define TW_TILE 1024u            // bytes of a row one trip of a wave covers: an aligned 16 bytes of the scratch per lane
#define TW_ZHEAD 2u              // the zlib header in front of a segment's first piece
#define TW_ZTAIL 4u              // the Adler-32 behind its last
#define TW_E_ARG (-103)

// where the pieces of segment k start in the table, and the segment of piece i
static __device__ __forceinline__ uint32_t tw_first(const zmi_tw_plan& g, uint32_t k) { return k < g.n_segs ? k * g.ppf : g.np; }
static __device__ __forceinline__ uint32_t tw_seg_of(const zmi_tw_plan& g, uint32_t i) {
    const uint32_t k = i / g.ppf;
    return k < g.n_segs ? k : g.n_segs - 1u;
}

// One thread per place of the table and one more.  p_off / p_len: the piece's bytes in the scratch; head: TW_ZHEAD in front of a
// segment's first piece, 0 elsewhere; the bit of a segment's last piece is set in `ends` (zeroed by the caller: wpg words for every
// launch group of `group` pieces); first[k]: the scan of the piece counts, n_segs + 1 words, for the fold of the Adler-32 values.
__global__ void __launch_bounds__(256) zmi_tiff_wpieces_kernel(zmi_tw_plan g, uint32_t group, uint32_t wpg, uint64_t* __restrict__ p_off,
                                                               uint32_t* __restrict__ p_len, uint32_t* __restrict__ head, uint32_t* ends,
                                                               uint64_t* __restrict__ first, uint32_t* __restrict__ n_eff,
                                                               uint64_t* __restrict__ pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u) { *n_eff = g.n_segs; pos[0] = g.seg0; }
    if (i <= g.n_segs) first[i] = tw_first(g, i);
    if (i >= g.np) return;
    const uint32_t k = tw_seg_of(g, i), q = i - k * g.ppf;
    const uint32_t l = k + 1u == g.n_segs ? g.last_bytes : g.seg_bytes;
    const uint64_t o = (uint64_t)q * g.piece_bytes;
    p_off[i] = (uint64_t)k * g.ss + o;
    p_len[i] = l - o < g.piece_bytes ? (uint32_t)(l - o) : g.piece_bytes;
    head[i] = q == 0u ? TW_ZHEAD : 0u;
    if (i + 1u == tw_first(g, k + 1u)) {
        const uint32_t j = i % group;
        atomicOr(&ends[(uint64_t)(i / group) * wpg + (j >> 5)], 1u << (j & 31u));
    }
}

// ---- the forward predictor (TIFF 6.0 section 14, Adobe Technical Note 3) --------------------------------------------------------------------
// A row of a segment is N = seg_w * samples samples of s bytes, rb = N * s bytes.  Predictor 1 copies; predictor 2 is d[i] = x[i] -
// x[i - samples] mod 2^(8 s), the first pixel as it is; predictor 3 puts byte b of sample k (b = 0 the most significant) to p[b * N + k]
// and takes q[j] = p[j] - p[j - samples] mod 256 over the row's bytes.  Unlike the undo nothing here is a scan: every output byte
// follows from two input samples, so the work is one read of the pixels and one write of the predicted bytes.
// The work item is (segment, band of plan.band_rows rows: about 8 KiB, 8 rows at most), one wave each, taken in turn by a fixed
// grid -- the geometry is uniform, so item / bands is the segment and no scan numbers them; the wave walks a row in trips of TW_TILE
// bytes.  A lane owns ONE ALIGNED 16 BYTES OF THE SCRATCH per trip: the segments stand at multiples of 16 and rb is a multiple of
// the sample size, so the row offset y of a lane's bytes is 16 * k - (the row's misalignment in the scratch), a multiple of s -- the
// 16 bytes are whole samples whatever the row length is, and the store is one dwordx4 per lane but for the first and last 16 bytes of
// a row, which are written dword- and byte-wise.  The operands -- the row at y and at y - (bytes of a pixel) -- are each five aligned
// dword loads joined by v_alignbyte (tw_ld16: the input stands at any alignment; every address depends on the lane -- a wave-uniform
// one may become a scalar load, which drops the low bits of a misaligned base); the second hits the lines the first
// brought in.  The pixel size is therefore only a distance between two loads and the kernel has no variant per pixel size; the
// subtraction is packed for 8- and 16-bit samples (pw_sub4 and its 16-bit form), a plain dword for 32, a pair for 64.  Bytes outside the
// valid part of the row read as 0 by a mask, which gives the first pixel its "left neighbour" and, in assemble mode, the zero padding
// of edge tiles: there the row is the segment's part of the image's row, nv = (the columns inside the image) * (bytes of a pixel)
// bytes of it are valid, none of a row below the image, and the cut, the crop and the padding are this kernel's loads.
// Predictor 3 is a gather: a lane owns four aligned dwords 256 bytes apart (for a fixed plane consecutive lanes then read samples
// 4 apart and write consecutive dwords), every output byte is two byte loads, the row's plane and sample index follow from one
// division per dword.  float32 rows of a multiple of four samples -- every tile of the usual float page -- take a path of their own
// that loads whole samples (tw_predict_row).
// Bounds: a dword is loaded only where it holds at least one valid byte of the row; stores write the row's own rb bytes.
struct tw_v16 { uint32_t w[4]; };
static __device__ __forceinline__ uint32_t tw_sub2(uint32_t x, uint32_t p) {
    return ((x | 0x80008000u) - (p & 0x7FFF7FFFu)) ^ ((x ^ ~p) & 0x80008000u);
}
// row[y .. y + 16) as four little-endian dwords, bytes outside [0, nv) as 0
// (IN: the caller knows [y - 3, y + 20) to lie inside [0, nv) -- no test, no mask)
template <bool IN>
static __device__ __forceinline__ tw_v16 tw_ld16(const uint8_t* row, int32_t y, int32_t nv) {
    const uint8_t* p = row + y;
    const uint32_t m = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - m);
    uint32_t a[5];
    tw_v16 r;
    if (IN) {
#pragma unroll
        for (uint32_t i = 0u; i < 5u; ++i) a[i] = q[i];
#pragma unroll
        for (uint32_t i = 0u; i < 4u; ++i) r.w[i] = __builtin_amdgcn_alignbyte(a[i + 1u], a[i], m);
        return r;
    }
    const int32_t q0 = y - (int32_t)m;                   // the row offset of q's first byte
#pragma unroll
    for (uint32_t i = 0u; i < 5u; ++i) {
        const int32_t lo = q0 + 4 * (int32_t)i;
        a[i] = (lo + 3 >= 0 && lo < nv && (i < 4u || m != 0u)) ? q[i] : 0u;
    }
#pragma unroll
    for (uint32_t i = 0u; i < 4u; ++i) r.w[i] = __builtin_amdgcn_alignbyte(a[i + 1u], a[i], m) & pw_mask(y + 4 * (int32_t)i, nv);
    return r;
}
// the 16 bytes of row offset y to dst + y (16-byte aligned), only the row's own bytes [0, rb)
template <bool IN>
static __device__ __forceinline__ void tw_st16(uint8_t* dst, int32_t y, int32_t rb, const tw_v16& v) {
    uint8_t* o = dst + y;
    if (IN || (y >= 0 && y + 16 <= rb)) {
        uint4 u;
        u.x = v.w[0]; u.y = v.w[1]; u.z = v.w[2]; u.w = v.w[3];
        *(uint4*)o = u;
        return;
    }
#pragma unroll
    for (uint32_t i = 0u; i < 4u; ++i) {
        const uint32_t vm = pw_mask(y + 4 * (int32_t)i, rb);
        if (vm == 0xFFFFFFFFu) ((uint32_t*)o)[i] = v.w[i];
        else if (vm != 0u) {
#pragma unroll
            for (uint32_t b = 0u; b < 4u; ++b)
                if ((vm >> (8u * b)) & 0xFFu) o[4u * i + b] = (uint8_t)(v.w[i] >> (8u * b));
        }
    }
}
// one trip of predictor 1 / 2 (S: bytes of a sample; pb: bytes of a pixel, 0 = predictor 1)
template <bool IN>
static __device__ __forceinline__ void tw_trip_diff(const uint8_t* src, int32_t nv, int32_t rb, int32_t pb, uint32_t S, int32_t y, uint8_t* dst) {
    if (!IN && (y + 16 <= 0 || y >= rb)) return;
    tw_v16 x = tw_ld16<IN>(src, y, nv);
    if (pb != 0) {
        const tw_v16 l = tw_ld16<IN>(src, y - pb, nv);
        if (S == 1u) {
#pragma unroll
            for (uint32_t i = 0u; i < 4u; ++i) x.w[i] = pw_sub4(x.w[i], l.w[i]);
        } else if (S == 2u) {
#pragma unroll
            for (uint32_t i = 0u; i < 4u; ++i) x.w[i] = tw_sub2(x.w[i], l.w[i]);
        } else if (S == 4u) {
#pragma unroll
            for (uint32_t i = 0u; i < 4u; ++i) x.w[i] -= l.w[i];
        } else {
#pragma unroll
            for (uint32_t i = 0u; i < 4u; i += 2u) {
                const uint64_t d = ((uint64_t)x.w[i + 1u] << 32 | x.w[i]) - ((uint64_t)l.w[i + 1u] << 32 | l.w[i]);
                x.w[i] = (uint32_t)d; x.w[i + 1u] = (uint32_t)(d >> 32);
            }
        }
    }
    tw_st16<IN>(dst, y, rb, x);
}
// one dword of predictor 3: the bytes q[y .. y + 4) of the row, those outside [0, rb) as 0.  N = samples of the row, S = bytes of a
// sample, spp = samples of a pixel
static __device__ __forceinline__ uint32_t tw_fp4(const uint8_t* src, int32_t nv, int32_t rb, uint32_t N, uint32_t S, uint32_t spp, int32_t y) {
    const int32_t j0 = y < 0 ? 0 : y;
    uint32_t b = (uint32_t)j0 / N, k = (uint32_t)j0 - b * N;
    uint32_t r = 0u;
    for (int32_t j = j0; j < y + 4 && j < rb; ++j) {
        const uint32_t ix = k * S + (S - 1u - b);
        const uint32_t v = (int32_t)ix < nv ? src[ix] : 0u;
        uint32_t l = 0u;
        if (b != 0u || k >= spp) {
            const uint32_t kl = k >= spp ? k - spp : k + N - spp, bl = k >= spp ? b : b - 1u;
            const uint32_t il = kl * S + (S - 1u - bl);
            l = (int32_t)il < nv ? src[il] : 0u;
        }
        r |= ((v - l) & 0xFFu) << (8u * (uint32_t)(j - y));
        if (++k == N) { k = 0u; ++b; }
    }
    return r;
}

// one row: src its first byte in the input (nv valid bytes, the rest of the rb read as 0), dst its rb bytes in the scratch.  A trip
// whose bytes lie four bytes and a pixel clear of both ends of the valid part (wave-uniform) needs no test and no mask: all but the
// first and last of a row
static __device__ __forceinline__ void tw_predict_row(const uint8_t* src, int32_t nv, int32_t rb, const zmi_tw_plan& g, uint8_t* dst, uint32_t lane) {
    const int32_t md = (int32_t)((uintptr_t)dst & 15u);
    if (g.pred == 3u && g.sb == 4u && ((g.seg_w * g.spp) & 3u) == 0u) {
        // float32 rows of a multiple of four samples (every tile): a lane loads four whole samples as predictor 2 would, with the four a
        // pixel to the left, picks plane b of both with shifts and stores one aligned dword per plane -- N is a multiple of 4 and so is
        // the row's place in the scratch.  The first pixel's left neighbours in the planes behind the first are the tail of the plane in
        // front: those lanes (the row's first one or two) take the general path
        const uint32_t N = g.seg_w * g.spp;
        for (uint32_t k0 = 0u; k0 < N; k0 += 256u) {
            const uint32_t k = k0 + 4u * lane;
            if (k >= N) continue;
            const int32_t y = 4 * (int32_t)k;
            const bool in = 4 * (int32_t)k0 - (int32_t)g.pb >= 4 && 4 * (int32_t)k0 + 1028 <= nv;     // (wave-uniform, as below)
            const tw_v16 x = in ? tw_ld16<true>(src, y, nv) : tw_ld16<false>(src, y, nv);
            const tw_v16 l = in ? tw_ld16<true>(src, y - (int32_t)g.pb, nv) : tw_ld16<false>(src, y - (int32_t)g.pb, nv);
#pragma unroll
            for (uint32_t b = 0u; b < 4u; ++b) {
                const uint32_t sh = 8u * (3u - b);
                const uint32_t pv = ((x.w[0] >> sh) & 0xFFu) | ((x.w[1] >> sh) & 0xFFu) << 8 | ((x.w[2] >> sh) & 0xFFu) << 16 | ((x.w[3] >> sh) & 0xFFu) << 24;
                const uint32_t pl = ((l.w[0] >> sh) & 0xFFu) | ((l.w[1] >> sh) & 0xFFu) << 8 | ((l.w[2] >> sh) & 0xFFu) << 16 | ((l.w[3] >> sh) & 0xFFu) << 24;
                uint32_t v = pw_sub4(pv, pl);
                if (k < g.spp && b != 0u) v = tw_fp4(src, nv, rb, N, 4u, g.spp, (int32_t)(b * N + k));
                *(uint32_t*)(dst + b * N + k) = v;
            }
        }
        return;
    }
    if (g.pred == 3u) {
        const uint32_t N = g.seg_w * g.spp;
        for (int32_t x0 = -md; x0 < rb; x0 += (int32_t)TW_TILE) {
#pragma unroll
            for (uint32_t i = 0u; i < 4u; ++i) {
                const int32_t y = x0 + 256 * (int32_t)i + 4 * (int32_t)lane;
                if (y + 4 <= 0 || y >= rb) continue;
                const uint32_t v = tw_fp4(src, nv, rb, N, g.sb, g.spp, y);
                const uint32_t vm = pw_mask(y, rb);
                uint8_t* o = dst + y;
                if (vm == 0xFFFFFFFFu) *(uint32_t*)o = v;
                else {
#pragma unroll
                    for (uint32_t b = 0u; b < 4u; ++b)
                        if ((vm >> (8u * b)) & 0xFFu) o[b] = (uint8_t)(v >> (8u * b));
                }
            }
        }
        return;
    }
    const int32_t pb = g.pred == 2u ? (int32_t)g.pb : 0;
    for (int32_t x0 = -md; x0 < rb; x0 += (int32_t)TW_TILE) {
        const int32_t y = x0 + 16 * (int32_t)lane;
        if (x0 - pb >= 4 && x0 + (int32_t)TW_TILE + 4 <= nv) tw_trip_diff<true>(src, nv, rb, pb, g.sb, y, dst);
        else tw_trip_diff<false>(src, nv, rb, pb, g.sb, y, dst);
    }
}

// dense: segment k is in[in_off[k] ..), its rows one behind the other; assemble: in is the [height, width, C] image
__global__ void __launch_bounds__(64) zmi_tiff_predict_kernel(zmi_tw_plan g, const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                              uint8_t* __restrict__ scan) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = (uint64_t)g.n_segs * g.bands;
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t k = (uint32_t)(it / g.bands), band = (uint32_t)(it - (uint64_t)k * g.bands);
        const uint32_t tx = k % g.across, ty = k / g.across;
        const uint32_t rows = k + 1u == g.n_segs ? g.last_bytes / g.rb : g.seg_h;
        const uint32_t r0 = band * g.band_rows, r1 = rows - r0 < g.band_rows ? rows : r0 + g.band_rows;
        if (r0 >= rows) continue;                        // (the last strip may have fewer bands than the others)
        uint8_t* dst = scan + (uint64_t)k * g.ss;
        const uint8_t* src;
        uint64_t pitch;
        uint32_t ow = g.seg_w, oh = rows;                // the columns and rows of the segment that are given
        if (g.assemble) {
            const uint32_t left_w = g.width - tx * g.seg_w, left_h = g.height - ty * g.seg_h;
            ow = left_w < g.seg_w ? left_w : g.seg_w;
            oh = left_h < rows ? left_h : rows;
            pitch = (uint64_t)g.width * g.pb;
            src = in + ((uint64_t)ty * g.seg_h * g.width + (uint64_t)tx * g.seg_w) * g.pb;
        } else {
            pitch = g.rb;
            src = in + in_off[k];
        }
        for (uint32_t r = r0; r < r1; ++r)
            tw_predict_row(src + (uint64_t)r * pitch, r < oh ? (int32_t)(ow * g.pb) : 0, (int32_t)g.rb, g, dst + (uint64_t)r * g.rb, lane);
    }
}

// zmi_png_place_kernel with the bytes behind a piece that ends a segment as a parameter: piece i of the group takes its hole, its
// payload and, where its bit in `ends` is set, `tail` bytes, behind which the running place is rounded up to align -- so every segment
// starts at a multiple of it, segment 0 at the one the host put into pos[0]
__global__ void __launch_bounds__(1024) zmi_tiff_place_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ olen,
                                                              const uint32_t* __restrict__ ends, uint32_t n, uint32_t align, uint32_t tail,
                                                              uint64_t* pos) {
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
        const pw_run one = {(uint64_t)head[i] + olen[i] + (e ? tail : 0u), 0ull, e ? 1u : 0u};
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
        pos[i] = p;
        p += (uint64_t)head[i] + olen[i] + (e ? tail : 0u);
        if (e) p = (p + am) & ~am;
    }
    if (t == 1023u) pos[n] = p;
}

// a byte of the file, where it lies in front of out_cap
static __device__ __forceinline__ void tw_put(uint8_t* out, uint64_t out_cap, uint64_t at, uint32_t b) {
    if (at < out_cap) out[at] = (uint8_t)b;
}
__global__ void __launch_bounds__(256) zmi_tiff_wmeta_kernel(zmi_tw_meta m, uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < m.a_len; i += 256u) tw_put(out, out_cap, i, m.b[i]);
    for (uint32_t i = t; i < m.b_len; i += 256u) tw_put(out, out_cap, m.b_pos + i, m.b[m.a_len + i]);
}

// where segment k starts and ends in the file, behind the last group's places
static __device__ __forceinline__ void tw_span(const zmi_tw_plan& g, const uint64_t* __restrict__ pos, const uint32_t* __restrict__ olen, uint32_t k,
                                               uint64_t* at, uint64_t* end) {
    const uint32_t p0 = tw_first(g, k), pl = tw_first(g, k + 1u) - 1u;
    *at = pos[p0];
    *end = pos[pl] + (pl == p0 ? TW_ZHEAD : 0u) + olen[pl] + TW_ZTAIL;
}
// One wave per segment, behind the last group: the zeros between the segment in front (segment 0: the metadata) and this one, the two
// bytes of the zlib header, the big-endian Adler-32, the segment's offset and byte count in the two arrays (LONG, BigTIFF LONG8), its
// length and its status -- the first encoder status of its pieces, which also goes into *bad as the least index of such a segment.
__global__ void __launch_bounds__(256) zmi_tiff_wsegs_kernel(zmi_tw_plan g, const uint64_t* __restrict__ pos, const uint32_t* __restrict__ olen,
                                                             const int32_t* __restrict__ st, const uint32_t* __restrict__ adler, uint32_t level,
                                                             uint32_t strategy, uint8_t* __restrict__ out, uint64_t out_cap,
                                                             uint32_t* __restrict__ seg_len, int32_t* __restrict__ status, uint32_t* bad) {
    const uint32_t lane = zmi_lane();
    const uint32_t k = blockIdx.x * 4u + zmi_wave();
    if (k >= g.n_segs) return;                           // (the whole wave)
    uint64_t at, end, front = g.meta_end, none;
    tw_span(g, pos, olen, k, &at, &end);
    if (k != 0u) tw_span(g, pos, olen, k - 1u, &none, &front);
    uint32_t fp = 0xFFFFFFFFu;                           // the least piece of the segment with a status: a lane's first, then the wave's
    for (uint32_t p = tw_first(g, k) + lane; p < tw_first(g, k + 1u) && fp == 0xFFFFFFFFu; p += 64u)
        if (st[p] != 0) fp = p;
    fp = ~zmi_wave_max(~fp);
    const int32_t es = fp != 0xFFFFFFFFu ? st[fp] : 0;
    for (uint64_t i = front + lane; i < at; i += 64u) tw_put(out, out_cap, i, 0u);
    uint8_t zh[10];
    zmi_stream_header(1u, level, strategy, zh);
    const uint32_t ad = adler[k], es8 = g.big ? 8u : 4u;
    const uint64_t cnt = end - at;
    if (lane < 2u) tw_put(out, out_cap, at + lane, zh[lane]);
    else if (lane < 6u) tw_put(out, out_cap, end - 6u + lane, ad >> (8u * (5u - lane)));
    else if (lane < 6u + es8) tw_put(out, out_cap, g.off_pos + (uint64_t)k * es8 + (lane - 6u), (uint32_t)(at >> (8u * (lane - 6u))));
    else if (lane < 6u + 2u * es8) tw_put(out, out_cap, g.cnt_pos + (uint64_t)k * es8 + (lane - 6u - es8), (uint32_t)(cnt >> (8u * (lane - 6u - es8))));
    if (lane == 0u) {
        if (seg_len) seg_len[k] = (uint32_t)cnt;
        status[k] = es;
        if (es != 0) atomicMin(bad, k);
    }
}

// the file's words (include/zmi355.h states the order of the statuses) and d_written: the record of the plan, or zeros with the status
__global__ void __launch_bounds__(64) zmi_tiff_wclose_kernel(zmi_tw_plan g, zmi_tw_meta m, const uint64_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ olen, const int32_t* __restrict__ status,
                                                             const uint32_t* __restrict__ bad, uint64_t out_cap, uint64_t* __restrict__ file_len,
                                                             int32_t* __restrict__ file_status, uint8_t* __restrict__ written) {
    const uint32_t t = threadIdx.x;
    uint64_t at, end;
    tw_span(g, pos, olen, g.n_segs - 1u, &at, &end);
    int32_t s = 0;
    if (!g.big && end > 0xFFFFFFFFull) s = TW_E_ARG;
    else if (end > out_cap) s = ZMI_BUF_ERROR;
    else if (*bad != 0xFFFFFFFFu) s = status[*bad];
    if (t == 0u) { *file_len = end; *file_status = s; }
    if (written) {
        for (uint32_t i = t; i < 72u; i += 64u) {
            uint32_t b = s == 0 ? m.rec[i] : 0u;
            if (s != 0 && i >= 68u) b = ((uint32_t)s >> (8u * (i - 68u))) & 0xFFu;
            written[i] = (uint8_t)b;
        }
    }
}

extern "C" uint32_t zmi_tiff_predict_tile(void) { return TW_TILE; }
extern "C" int zmi_launch_tiff_wpieces(zmi_tw_plan plan, uint32_t group, uint32_t wpg, uint64_t* d_p_off, uint32_t* d_p_len, uint32_t* d_head,
                                       uint32_t* d_ends, uint64_t* d_first, uint32_t* d_n_eff, uint64_t* d_pos, hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_wpieces_kernel, dim3(plan.np / 256u + 1u), dim3(256), 0, stream, plan, group, wpg, d_p_off, d_p_len, d_head, d_ends, d_first,
               d_n_eff, d_pos);
    return 0;
}
// a fixed grid takes the items in turn: a few waves per SIMD
extern "C" int zmi_launch_tiff_predict(zmi_tw_plan plan, const uint8_t* d_in, const uint64_t* d_in_off, uint8_t* d_scan, hipStream_t stream) {
    const uint64_t items = (uint64_t)plan.n_segs * plan.bands;
    const uint32_t grid = items < 32768ull ? (uint32_t)items : 32768u;
    ZMI_LAUNCH(zmi_tiff_predict_kernel, dim3(grid), dim3(64), 0, stream, plan, d_in, d_in_off, d_scan);
    return 0;
}
extern "C" int zmi_launch_tiff_place(const uint32_t* d_head, const uint32_t* d_olen, const uint32_t* d_ends, uint32_t n, uint32_t align, uint64_t* d_pos,
                                     hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_place_kernel, dim3(1), dim3(1024), 0, stream, d_head, d_olen, d_ends, n, align, TW_ZTAIL, d_pos);
    return 0;
}
extern "C" int zmi_launch_tiff_wmeta(zmi_tw_meta meta, uint8_t* d_out, uint64_t out_cap, hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_wmeta_kernel, dim3(1), dim3(256), 0, stream, meta, d_out, out_cap);
    return 0;
}
extern "C" int zmi_launch_tiff_wsegs(zmi_tw_plan plan, const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_st, const uint32_t* d_adler,
                                     uint32_t level, uint32_t strategy, uint8_t* d_out, uint64_t out_cap, uint32_t* d_seg_len, int32_t* d_status,
                                     uint32_t* d_bad, hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_wsegs_kernel, dim3((plan.n_segs + 3u) / 4u), dim3(256), 0, stream, plan, d_pos, d_olen, d_st, d_adler, level, strategy, d_out,
               out_cap, d_seg_len, d_status, d_bad);
    return 0;
}
extern "C" int zmi_launch_tiff_wclose(zmi_tw_plan plan, zmi_tw_meta meta, const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_status,
                                      const uint32_t* d_bad, uint64_t out_cap, uint64_t* d_file_len, int32_t* d_file_status, void* d_written,
                                      hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_wclose_kernel, dim3(1), dim3(64), 0, stream, plan, meta, d_pos, d_olen, d_status, d_bad, out_cap, d_file_len, d_file_status,
               (uint8_t*)d_written);
    return 0;
}
