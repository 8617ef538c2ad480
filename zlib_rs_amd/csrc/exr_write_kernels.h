// exr_write_kernels.h -- writing OpenEXR images with ZIP / ZIPS / PXR24 / NONE compression (zmi_exr_write_dev; every byte of the file:
// include/zmi355.h); included by pack.hip behind exr_kernels.h, whose helpers (xr_find, xr_perm, xr_type_bytes) it uses.
//
// A batch of images of ONE layout: the layout is the caller's, so the plan (zmi_xw_plan, zmi_kernels.h) is worked out on the host and
// every kernel takes it by value; the channel records and the header's bytes reach the scratch in kernel arguments (zmi_exr_wslice_kernel).
// Only the compressed sizes are device values.  A chunk's raw bytes run through the forward zip into context scratch, are cut into
// pieces of piece_bytes and join ONE piece table that the independent-piece encoder works through in launch groups of whole chunks, as
// the segments of zmi_tiff_write_dev do; the payload copies are zmi_zip_pack_kernel.  What no other writer has is the store-raw rule: a
// chunk whose candidate stream is not shorter than its n raw bytes is stored raw, so a chunk's place follows from the decision.  The kernels:
//   zmi_exr_wchunks_kernel   one thread per chunk of the call: raw size, pieces, room in the scratch, work items (their scans follow)
//   zmi_exr_wpieces_kernel   the piece table: piece p belongs to the chunk the scan of the piece counts names, by bisection
//   zmi_exr_zip_kernel       the hot path, below
//   zmi_exr_pxr24_forward_kernel   its place under PXR24: d is m bytes of byte planes, everything behind it runs with m where ZIP has n
//   zmi_exr_wplace_kernel    one launch group: every chunk's candidate length, the raw decision, its dataSize and its place -- a scan
//                            over (size, ends a file) pairs, the running offset a device word --, its pieces' places
//   zmi_exr_gather_kernel    the raw chunks (all of them under NONE): the runs from the planes straight to their place in the file
//   zmi_exr_whead_kernel / zmi_exr_wframe_kernel   the header's bytes; per chunk its table entry, its header, the zlib header and the Adler-32
//   zmi_exr_wwords_kernel    the images' words, d_written and d_written_channels
#pragma once

#define XW_TRIP 2048u                // raw bytes of one trip of a wave: 64 lanes x 32 bytes, 16 to each of the two streams
#define XW_PIECE (4u * XW_TRIP)      // the longest piece of a run one work item reads
#define XW_VOID 0xFFFFFFFFu          // head[] of a piece zmi_zip_pack_kernel leaves alone (ZW_VOID): a piece of a chunk stored raw
#define XW_P24_TRIP 256u             // pixels of one trip of the PXR24 forward: 64 lanes x 4 (EXR_P24_TRIP of the reader)

struct xw_box { uint32_t x0, y0, cw, rows, tx, ty; };
static __device__ __forceinline__ void xw_box_of(const zmi_xw_plan& g, uint32_t k, xw_box* b) {
    b->tx = k % g.across; b->ty = k / g.across;
    b->x0 = b->tx * g.box_w; b->y0 = b->ty * g.box_h;
    b->cw = g.W - b->x0 < g.box_w ? g.W - b->x0 : g.box_w;
    b->rows = g.H - b->y0 < g.box_h ? g.H - b->y0 : g.box_h;
}
// the pieces of at most XW_PIECE bytes that the runs of one row of a box cw pixels wide are cut into
static __device__ __forceinline__ uint32_t xw_row_items(const zmi_xw_plan& g, const zmi_exr_channel* __restrict__ chs, uint32_t cw) {
    uint32_t per_row = 0u;
    for (uint32_t x = 0u; x < g.n_ch; ++x) per_row += (cw * xr_type_bytes(chs[x].pixel_type) + XW_PIECE - 1u) / XW_PIECE;
    return per_row;
}

__global__ void __launch_bounds__(256) zmi_exr_wslice_kernel(zmi_xw_slice s, uint8_t* __restrict__ blob) {
    for (uint32_t i = threadIdx.x; i < s.len; i += 256u) blob[s.at + i] = s.b[i];
}

// csz = the chunk's raw size n; npc = its pieces and ssz = its room in the scratch, n rounded up to 16 (both 0 under NONE: nothing is
// encoded); items = the work items of its runs; cds = n, the dataSize of a chunk stored raw, until the place kernel decides.  The words
// the later kernels start from: *n_eff = the chunks (the fold of the Adler-32 values), bad[i] = no piece of image i has a status,
// run[0] = 0, where the first file starts.
// PXR24 (compression 5): cm = the bytes m of the chunk's d -- rows * cw * per_p, where ZIP has n; pieces and room follow m -- and
// fitems = the trips of its runs, the work items of zmi_exr_pxr24_forward_kernel (0 otherwise).
__global__ void __launch_bounds__(256) zmi_exr_wchunks_kernel(zmi_xw_plan g, const zmi_exr_channel* __restrict__ chs, uint32_t* __restrict__ csz,
                                                              uint32_t* __restrict__ npc, uint32_t* __restrict__ ssz, uint32_t* __restrict__ items,
                                                              uint32_t* __restrict__ cds, uint32_t* __restrict__ n_eff, uint32_t* __restrict__ bad,
                                                              uint64_t* __restrict__ run, uint32_t* __restrict__ cm, uint32_t* __restrict__ fitems) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q == 0u) { *n_eff = g.ncc; run[0] = 0ull; }
    if (q >= g.ncc) return;
    const uint32_t img = q / g.nc, k = q - img * g.nc;
    if (k == 0u) bad[img] = 0xFFFFFFFFu;
    xw_box b;
    xw_box_of(g, k, &b);
    const uint32_t n = b.rows * b.cw * g.per_px;
    const uint32_t m = g.comp == 5u ? b.rows * b.cw * g.per_p : n;
    csz[q] = n; cds[q] = n; cm[q] = m;
    npc[q] = g.comp == 0u ? 0u : (uint32_t)(((uint64_t)m + g.piece_bytes - 1u) / g.piece_bytes);
    ssz[q] = g.comp == 0u ? 0u : (uint32_t)(((uint64_t)m + 15ull) & ~15ull);
    items[q] = b.rows * xw_row_items(g, chs, b.cw);
    fitems[q] = g.comp == 5u ? b.rows * g.n_ch * ((b.cw + XW_P24_TRIP - 1u) / XW_P24_TRIP) : 0u;
}

// One thread per piece.  p_off / p_len: the piece's bytes in the scratch; the bit of a chunk's last piece is set in `ends` (zeroed by
// the caller): wpg words for every launch group of group_chunks chunks, bit = the piece's index behind the group's first piece.
__global__ void __launch_bounds__(256) zmi_exr_wpieces_kernel(zmi_xw_plan g, const uint64_t* __restrict__ cfirst, const uint64_t* __restrict__ soff,
                                                              const uint32_t* __restrict__ csz, uint32_t group_chunks, uint32_t wpg, uint32_t np,
                                                              uint64_t* __restrict__ p_off, uint32_t* __restrict__ p_len, uint32_t* ends) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= np) return;
    const uint32_t q = xr_find(cfirst, g.ncc, p);
    const uint32_t j = p - (uint32_t)cfirst[q], n = csz[q];
    const uint64_t o = (uint64_t)j * g.piece_bytes;
    p_off[p] = soff[q] + o;
    p_len[p] = n - o < g.piece_bytes ? (uint32_t)(n - o) : g.piece_bytes;
    if ((uint64_t)p + 1u == cfirst[q + 1u]) {
        const uint32_t grp = q / group_chunks, bit = p - (uint32_t)cfirst[grp * group_chunks];
        atomicOr(&ends[(uint64_t)grp * wpg + (bit >> 5)], 1u << (bit & 31u));
    }
}

// ---- the forward zip (the interleave and the predictor of a ZIP / ZIPS chunk) and the raw gather ---------------------------------------------
// The chunk's raw bytes raw[0 .. n) are its rows, every row the planar runs of its channels; n is even (a pixel is 2 or 4 bytes).  With
// h = n / 2: t[i] = raw[2 i], t[h + i] = raw[2 i + 1], d[0] = t[0], d[i] = (t[i] - t[i - 1] + 128) mod 256.  Nothing here is a scan:
// every byte of d follows from two raw bytes two apart, except d[h], which needs raw[1] and raw[n - 2].
// The work item mirrors the reader's unzip: a piece of at most XW_PIECE bytes of a (chunk, row, channel) run, read from the channel's
// plane, the items numbered by the scan of the chunks' counts and taken in turn by a fixed grid of one-wave workgroups.  The piece is
// raw[a .. a + len), a and len even, so it gives d[a / 2 ..) and d[h + a / 2 ..), len / 2 bytes each.  A trip is XW_TRIP raw bytes: a
// lane loads its 32 as aligned dwords joined by v_alignbyte (every address depends on the lane -- a wave-uniform misaligned address may
// become a scalar load that drops the low bits, DESIGN.md section 22 --, and a dword is loaded only where it holds a byte of the piece),
// splits them with v_perm_b32 into 16 even and 16 odd bytes, shifts each stream by one byte to get the predecessors -- the byte in
// front of the lane's first comes from the lane below (DPP), in front of lane 0's from the trip before, in front of the item from ONE
// extra load: the pair raw[a - 2], raw[a - 1] ends the run in front (the same run, the channel in front, or the last channel of the row
// above), and the item at a = 0 takes raw[n - 2] for d[h] and no predecessor for d[0] -- and subtracts with +128 folded in on 00FF00FF
// fields, where no borrow crosses into a neighbour byte.  The two streams' destinations differ by h, which is seldom a multiple of
// 16, and start at a / 2: a lane's 16 bytes go out as one dwordx4 where they stand at a multiple of 16, as four dwords at a multiple
// of 4, and otherwise as up to three bytes, three dwords joined by v_alignbyte and the remaining bytes; a lane with fewer than 16 stores
// bytes.  No LDS.
// Bounds: loads touch the dwords that hold a lane's own bytes only; stores write d[0 .. n) of the chunk, which stands in the scratch
// at a multiple of 16.
static __device__ __forceinline__ uint32_t xw_diff4(uint32_t x, uint32_t p) {
    const uint32_t m = 0x00FF00FFu;
    const uint32_t lo = ((x & m) + 0x01800180u - (p & m)) & m;
    const uint32_t hi = (((x >> 8) & m) + 0x01800180u - ((p >> 8) & m)) & m;
    return lo | hi << 8;
}
// w[0 .. 8) = the ov <= 32 bytes at p (any alignment); what stands behind them in w is not used
static __device__ __forceinline__ void xw_ld32(const uint8_t* p, uint32_t ov, uint32_t* w) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - mis);
    const uint32_t ndw = ov != 0u ? (mis + ov + 3u) >> 2 : 0u;
    uint32_t d[9];
#pragma unroll
    for (uint32_t k = 0u; k < 9u; ++k) d[k] = k < ndw ? q[k] : 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 8u; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1u], d[k], mis);
}
// the first v <= 16 bytes of w[0 .. 4) to p (any alignment)
static __device__ __forceinline__ void xw_st16(uint8_t* p, const uint32_t* w, uint32_t v) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    if (v == 16u) {
        if (((uintptr_t)p & 15u) == 0u) {
            uint4 u;
            u.x = w[0]; u.y = w[1]; u.z = w[2]; u.w = w[3];
            *(uint4*)p = u;
        } else if (mis == 0u) {
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) ((uint32_t*)p)[k] = w[k];
        } else {
            const uint32_t hb = 4u - mis;                 // the bytes in front of the first aligned dword
#pragma unroll
            for (uint32_t b = 0u; b < 3u; ++b)
                if (b < hb) p[b] = (uint8_t)(w[0] >> (8u * b));
            uint32_t* q = (uint32_t*)(p + hb);
#pragma unroll
            for (uint32_t k = 0u; k < 3u; ++k) q[k] = __builtin_amdgcn_alignbyte(w[k + 1u], w[k], hb);
#pragma unroll
            for (uint32_t b = 0u; b < 3u; ++b)
                if (b < mis) p[hb + 12u + b] = (uint8_t)(w[3] >> (8u * (hb + b)));
        }
        return;
    }
#pragma unroll
    for (uint32_t b = 0u; b < 16u; ++b)
        if (b < v) p[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
}

// Work item `it` of the call: the piece raw[a .. a + len) of chunk q (n raw bytes) at src; pair = where the two raw bytes in front of
// it stand -- for a = 0 the chunk's last two.
struct xw_item {
    uint32_t q, n, a, len;
    const uint8_t *src, *pair;
};
static __device__ __forceinline__ void xw_item_of(const zmi_xw_plan& g, const zmi_exr_channel* __restrict__ chs, const uint8_t* __restrict__ in,
                                                  const uint64_t* __restrict__ in_off, const uint64_t* __restrict__ item_off, uint64_t it,
                                                  xw_item* o) {
    const uint32_t q = xr_find(item_off, g.ncc, it);
    const uint32_t idx = (uint32_t)(it - item_off[q]);
    const uint32_t img = q / g.nc;
    xw_box b;
    xw_box_of(g, q - img * g.nc, &b);
    const uint32_t per_row = xw_row_items(g, chs, b.cw), rb = b.cw * g.per_px;
    const uint32_t row = idx / per_row;
    uint32_t rem = idx % per_row, x = 0u, choff = 0u;
    for (;; ++x) {
        const uint32_t run = b.cw * xr_type_bytes(chs[x].pixel_type);
        const uint32_t pieces = (run + XW_PIECE - 1u) / XW_PIECE;
        if (rem < pieces || x + 1u == g.n_ch) break;
        rem -= pieces; choff += run;
    }
    const uint32_t size = xr_type_bytes(chs[x].pixel_type);
    const uint32_t run = b.cw * size, p0 = rem * XW_PIECE;
    const uint8_t* base = in + in_off[img];
    o->q = q;
    o->n = b.rows * rb;
    o->len = run - p0 < XW_PIECE ? run - p0 : XW_PIECE;
    o->a = row * rb + choff + p0;
    o->src = base + chs[x].plane_off + ((uint64_t)(b.y0 + row) * g.W + b.x0) * size + p0;
    if (o->a != 0u && p0 != 0u) { o->pair = o->src - 2; return; }
    uint32_t xl = g.n_ch - 1u, rl = b.rows - 1u;         // a = 0: the end of the chunk
    if (o->a != 0u) {
        if (x != 0u) { xl = x - 1u; rl = row; }
        else rl = row - 1u;
    }
    const uint32_t sl = xr_type_bytes(chs[xl].pixel_type);
    o->pair = base + chs[xl].plane_off + ((uint64_t)(b.y0 + rl) * g.W + b.x0 + b.cw) * sl - 2;
}

__global__ void __launch_bounds__(64) zmi_exr_zip_kernel(zmi_xw_plan g, const zmi_exr_channel* __restrict__ chs, const uint8_t* __restrict__ in,
                                                         const uint64_t* __restrict__ in_off, const uint64_t* __restrict__ item_off,
                                                         const uint64_t* __restrict__ soff, uint8_t* __restrict__ scan) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[g.ncc];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        xw_item m;
        xw_item_of(g, chs, in, in_off, item_off, it, &m);
        uint32_t pr = 0u;
        if (lane == 0u) pr = (uint32_t)m.pair[0] | (uint32_t)m.pair[1] << 8;
        pr = zmi_readlane(pr, 0u);
        // the bytes in front of the two streams: d[0] = t[0] is t[0] - 128 + 128
        uint32_t ca = m.a != 0u ? (pr & 0xFFu) : 128u, cb = m.a != 0u ? pr >> 8 : (pr & 0xFFu);
        uint8_t* da = scan + soff[m.q] + m.a / 2u;
        uint8_t* db = da + m.n / 2u;
        for (uint32_t t0 = 0u; t0 < m.len; t0 += XW_TRIP) {
            const uint32_t left = m.len - t0 < XW_TRIP ? m.len - t0 : XW_TRIP;
            const uint32_t ov = 32u * lane < left ? (left - 32u * lane < 32u ? left - 32u * lane : 32u) : 0u;
            uint32_t w[8], e[4], o[4], de[4], dd[4];
            xw_ld32(m.src + t0 + 32u * lane, ov, w);
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) {
                e[k] = xr_perm(w[2u * k + 1u], w[2u * k], 0x06040200u);
                o[k] = xr_perm(w[2u * k + 1u], w[2u * k], 0x07050301u);
            }
            // (a lane with bytes has a full lane below it)
            const uint32_t ue = zmi_lane_up1(e[3]) >> 24, uo = zmi_lane_up1(o[3]) >> 24;
            const uint32_t pe = lane == 0u ? ca : ue, po = lane == 0u ? cb : uo;
            de[0] = xw_diff4(e[0], e[0] << 8 | pe);
            dd[0] = xw_diff4(o[0], o[0] << 8 | po);
#pragma unroll
            for (uint32_t k = 1u; k < 4u; ++k) {
                de[k] = xw_diff4(e[k], __builtin_amdgcn_alignbyte(e[k], e[k - 1u], 3u));
                dd[k] = xw_diff4(o[k], __builtin_amdgcn_alignbyte(o[k], o[k - 1u], 3u));
            }
            if (ov != 0u) {
                xw_st16(da + t0 / 2u + 16u * lane, de, ov / 2u);
                xw_st16(db + t0 / 2u + 16u * lane, dd, ov / 2u);
            }
            ca = zmi_readlane(e[3], 63u) >> 24;
            cb = zmi_readlane(o[3], 63u) >> 24;
        }
    }
}

// The same items, for the chunks whose dataSize is n: the piece goes from its plane to cpos[q] + chdr + a.  A chunk that crosses
// out_cap is not written at all (its file's status says so).
__global__ void __launch_bounds__(64) zmi_exr_gather_kernel(zmi_xw_plan g, const zmi_exr_channel* __restrict__ chs, const uint8_t* __restrict__ in,
                                                            const uint64_t* __restrict__ in_off, const uint64_t* __restrict__ item_off,
                                                            const uint32_t* __restrict__ csz, const uint32_t* __restrict__ cds,
                                                            const uint64_t* __restrict__ cpos, uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[g.ncc];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t q = xr_find(item_off, g.ncc, it);
        const uint64_t at = cpos[q] + g.chdr;
        if (cds[q] != csz[q] || at + csz[q] > out_cap) continue;
        xw_item m;
        xw_item_of(g, chs, in, in_off, item_off, it, &m);
        uint8_t* dst = out + at + m.a;
        for (uint32_t t0 = 0u; t0 < m.len; t0 += XW_TRIP) {
            const uint32_t left = m.len - t0 < XW_TRIP ? m.len - t0 : XW_TRIP;
            if (32u * lane >= left) continue;
            const uint32_t ov = left - 32u * lane < 32u ? left - 32u * lane : 32u;
            uint32_t w[8];
            xw_ld32(m.src + t0 + 32u * lane, ov, w);
            xw_st16(dst + t0 + 32u * lane, w, ov < 16u ? ov : 16u);
            if (ov > 16u) xw_st16(dst + t0 + 32u * lane + 16u, w + 4, ov - 16u);
        }
    }
}

// ---- the PXR24 forward (compression 5; include/zmi355.h states the layout) --------------------------------------------------------------------
// d of a chunk is, for every row and channel, a run of p planes of cw bytes (p = 2 / 3 / 4 for HALF / FLOAT / UINT), most significant
// first, that hold diff[x] = v[x] - v[x - 1] mod 2^(8p), v[-1] = 0, v = the sample (a FLOAT rounded to 24 bits, xw_f24).  Nothing here
// is a scan: the work item is one trip of XW_P24_TRIP pixels of a (chunk, row, channel) run, every run of a chunk has the same number
// of trips, so an item's place follows by division.  A lane loads its 4 consecutive pixels from the plane (xr_ld16: aligned dwords
// joined by v_alignbyte, every address lane-dependent), takes the predecessor of its first from the lane below (DPP) -- lane 0 loads
// the pixel in front of the trip with byte loads, and has 0 at the start of a run --, subtracts, splits the four differences into
// byte planes with v_perm_b32 and stores 4 bytes to each plane: a dword where they stand 4-aligned, bytes otherwise (a plane starts at
// any byte offset of d).  Bounds: loads touch the dwords that hold a lane's own bytes only; stores write d[0 .. m) of the chunk.
static __device__ __forceinline__ uint32_t xw_f24(uint32_t u) {
    const uint32_t s = u & 0x80000000u, e = u & 0x7F800000u;
    uint32_t m = u & 0x007FFFFFu, i;
    if (e == 0x7F800000u) {
        if (m != 0u) { m >>= 8; i = (e >> 8) | m | (m == 0u ? 1u : 0u); }      // a NaN stays a NaN
        else i = e >> 8;
    } else {
        i = ((e | m) + (m & 0x80u)) >> 8;
        if (i >= 0x7F8000u) i = (e | m) >> 8;                                   // rounding never produces an infinity
    }
    return (s >> 8) | i;
}

__global__ void __launch_bounds__(64) zmi_exr_pxr24_forward_kernel(zmi_xw_plan g, const zmi_exr_channel* __restrict__ chs,
                                                                   const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                   const uint64_t* __restrict__ fitem_off, const uint64_t* __restrict__ soff,
                                                                   uint8_t* __restrict__ scan) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = fitem_off[g.ncc];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t q = xr_find(fitem_off, g.ncc, it);
        const uint32_t idx = (uint32_t)(it - fitem_off[q]);
        const uint32_t img = q / g.nc;
        xw_box b;
        xw_box_of(g, q - img * g.nc, &b);
        const uint32_t tp = (b.cw + XW_P24_TRIP - 1u) / XW_P24_TRIP;
        const uint32_t row = idx / (g.n_ch * tp), x = (idx / tp) % g.n_ch, t0 = (idx % tp) * XW_P24_TRIP;
        uint32_t choff = 0u;
        for (uint32_t y = 0u; y < x; ++y) choff += b.cw * xr_p24_bytes(chs[y].pixel_type);
        const int32_t type = chs[x].pixel_type;
        const uint32_t p = xr_p24_bytes(type), size = xr_type_bytes(type), w = b.cw;
        const uint32_t mask = p == 4u ? 0xFFFFFFFFu : (1u << (8u * p)) - 1u;
        const uint8_t* src = in + in_off[img] + chs[x].plane_off + ((uint64_t)(b.y0 + row) * g.W + b.x0) * size;
        uint8_t* dst = scan + soff[q] + (uint64_t)row * w * g.per_p + choff;
        const uint32_t left = w - t0 < XW_P24_TRIP ? w - t0 : XW_P24_TRIP;
        const uint32_t v = 4u * lane < left ? (left - 4u * lane < 4u ? left - 4u * lane : 4u) : 0u;
        const uint32_t px = t0 + 4u * lane;
        uint32_t ld[4] = {0u, 0u, 0u, 0u}, val[4];
        if (v != 0u) xr_ld16(src + (uint64_t)px * size, v * size, ld);
        uint32_t front = 0u;                                  // the pixel in front of the trip: lane 0 alone loads it
        if (lane == 0u && t0 != 0u) {
            const uint8_t* f = src + (uint64_t)(t0 - 1u) * size;
            front = (uint32_t)f[0] | (uint32_t)f[1] << 8;
            if (size == 4u) front |= (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
        }
        if (size == 2u) {
            val[0] = ld[0] & 0xFFFFu; val[1] = ld[0] >> 16; val[2] = ld[1] & 0xFFFFu; val[3] = ld[1] >> 16;
        } else {
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) val[k] = type == 2 ? xw_f24(ld[k]) : ld[k];
            if (type == 2) front = xw_f24(front);
        }
        // (a lane with pixels has a full lane below it)
        const uint32_t up = zmi_lane_up1(val[3]);
        const uint32_t prev = lane == 0u ? front : up;
        uint32_t d[4];
        d[0] = (val[0] - prev) & mask;
#pragma unroll
        for (uint32_t k = 1u; k < 4u; ++k) d[k] = (val[k] - val[k - 1u]) & mask;
        const uint32_t t01 = xr_perm(d[1], d[0], 0x05010400u), u01 = xr_perm(d[1], d[0], 0x07030602u);
        const uint32_t t23 = xr_perm(d[3], d[2], 0x05010400u), u23 = xr_perm(d[3], d[2], 0x07030602u);
        // b0 .. b3: the planes of bits 24 - 31 .. 0 - 7
        const uint32_t b3 = xr_perm(t23, t01, 0x05040100u), b2 = xr_perm(t23, t01, 0x07060302u);
        const uint32_t b1 = xr_perm(u23, u01, 0x05040100u), b0 = xr_perm(u23, u01, 0x07060302u);
        uint32_t a[4];
        a[0] = p == 4u ? b0 : (p == 3u ? b1 : b2);
        a[1] = p == 4u ? b1 : (p == 3u ? b2 : b3);
        a[2] = p == 4u ? b2 : b3;
        a[3] = b3;
#pragma unroll
        for (uint32_t k = 0u; k < 4u; ++k) {
            if (k >= p || v == 0u) continue;
            uint8_t* o = dst + (uint64_t)k * w + px;
            if (v == 4u && ((uintptr_t)o & 3u) == 0u) *(uint32_t*)o = a[k];
            else {
#pragma unroll
                for (uint32_t i = 0u; i < 4u; ++i)
                    if (i < v) o[i] = (uint8_t)(a[k] >> (8u * i));
            }
        }
    }
}

// One launch group: chunks first .. first + n of the call, whose pieces the encoder has just left in their slots.  A chunk's candidate
// is the zlib header, its pieces' payloads and the Adler-32; it is stored raw -- dataSize = n -- where that is not shorter than n, or
// where a piece has a status (bad[image] = the least such piece).  A chunk takes its header and its data, an image's first chunk the
// file's header and offset table in front, and behind an image's last chunk the running place is rounded up to out_align: the scan of
// zmi_tiff_place_kernel over chunks.  run[0] = where the group starts, run[1] = where the next one does.  cpos = the chunk's header in
// d_out; out_off[i] = where image i starts (out_off[n_images]: behind the last group); p_pos / head = the places of the pieces of a
// compressed chunk, XW_VOID for those of a raw one.
__global__ void __launch_bounds__(1024) zmi_exr_wplace_kernel(zmi_xw_plan g, uint32_t first, uint32_t n, const uint64_t* __restrict__ cfirst,
                                                              const uint32_t* __restrict__ csz, const uint32_t* __restrict__ olen,
                                                              const int32_t* __restrict__ st, uint64_t* run, uint32_t* __restrict__ cds,
                                                              uint64_t* __restrict__ cpos, uint64_t* __restrict__ p_pos, uint32_t* __restrict__ head,
                                                              uint64_t* __restrict__ out_off, uint32_t* bad) {
    __shared__ uint64_t sa[1024], sb[1024];
    __shared__ uint32_t sr[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t am = (uint64_t)g.out_align - 1u;
    const uint64_t base = run[0];
    const uint64_t pre = (uint64_t)g.hdr_len + 8ull * g.nc;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    pw_run mine = {0ull, 0ull, 0u};
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t q = first + i, k = q % g.nc, sz = csz[q];
        uint32_t ds = sz;
        if (g.comp != 0u) {
            uint64_t cand = 6ull;
            bool fail = false;
            for (uint64_t p = cfirst[q]; p < cfirst[q + 1u]; ++p) {
                cand += olen[p];
                if (st[p] != 0) { fail = true; atomicMin(&bad[q / g.nc], (uint32_t)p); }
            }
            if (!fail && cand < (uint64_t)sz) ds = (uint32_t)cand;
        }
        cds[q] = ds;
        const pw_run one = {(k == 0u ? pre : 0ull) + g.chdr + ds, 0ull, k + 1u == g.nc ? 1u : 0u};
        mine = pw_then(mine, one, am);
    }
    sa[t] = mine.a; sb[t] = mine.b; sr[t] = mine.r;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        pw_run f = {0ull, 0ull, 0u};
        if (t >= d) { f.a = sa[t - d]; f.b = sb[t - d]; f.r = sr[t - d]; }
        __syncthreads();
        if (t >= d) {
            pw_run h = {sa[t], sb[t], sr[t]};
            h = pw_then(f, h, am);
            sa[t] = h.a; sb[t] = h.b; sr[t] = h.r;
        }
        __syncthreads();
    }
    uint64_t p = base;
    if (t > 0u) p = sr[t - 1u] ? ((base + sa[t - 1u] + am) & ~am) + sb[t - 1u] : base + sa[t - 1u];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t q = first + i, k = q % g.nc, ds = cds[q];
        if (k == 0u) { out_off[q / g.nc] = p; p += pre; }
        cpos[q] = p;
        if (g.comp != 0u) {
            const bool raw = ds == csz[q];
            uint64_t at = p + g.chdr + 2u;
            for (uint64_t j = cfirst[q]; j < cfirst[q + 1u]; ++j) {
                p_pos[j] = at;
                head[j] = raw ? XW_VOID : 0u;
                at += olen[j];
            }
        }
        p += (uint64_t)g.chdr + ds;
        if (k + 1u == g.nc) p = (p + am) & ~am;
    }
    if (t == 1023u) {
        run[1] = p;
        if (first + n == g.ncc) out_off[g.n_images] = p;
    }
}

// a byte of a file, where it lies in front of out_cap
static __device__ __forceinline__ void xw_put(uint8_t* out, uint64_t out_cap, uint64_t at, uint32_t b) {
    if (at < out_cap) out[at] = (uint8_t)b;
}
static __device__ __forceinline__ void xw_put32(uint8_t* out, uint64_t out_cap, uint64_t at, uint32_t v) {
#pragma unroll
    for (uint32_t b = 0u; b < 4u; ++b) xw_put(out, out_cap, at + b, v >> (8u * b));
}
// one workgroup per image: the header's bytes, which the host made from *w
__global__ void __launch_bounds__(256) zmi_exr_whead_kernel(zmi_xw_plan g, const uint8_t* __restrict__ hdr, const uint64_t* __restrict__ out_off,
                                                            uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint64_t fs = out_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < g.hdr_len; i += 256u) xw_put(out, out_cap, fs + i, hdr[i]);
}
// one thread per chunk of the call, behind the last group, 64-bit positions: the chunk's entry in its file's offset table, its header
// -- the absolute y | tile x, tile y, level 0, 0 -- and dataSize, and around a compressed chunk's payload the two bytes of the zlib
// header and the big-endian Adler-32 of its d
__global__ void __launch_bounds__(256) zmi_exr_wframe_kernel(zmi_xw_plan g, const uint32_t* __restrict__ csz, const uint32_t* __restrict__ cds,
                                                             const uint64_t* __restrict__ cpos, const uint32_t* __restrict__ cadler,
                                                             const uint64_t* __restrict__ out_off, uint32_t level, uint32_t strategy,
                                                             uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= g.ncc) return;
    const uint32_t img = q / g.nc, k = q - img * g.nc, ds = cds[q];
    const uint64_t fs = out_off[img], cp = cpos[q], rel = cp - fs;
    xw_box b;
    xw_box_of(g, k, &b);
    const uint64_t te = fs + g.hdr_len + 8ull * k;
    xw_put32(out, out_cap, te, (uint32_t)rel);
    xw_put32(out, out_cap, te + 4u, (uint32_t)(rel >> 32));
    if (g.tiled) {
        xw_put32(out, out_cap, cp, b.tx);
        xw_put32(out, out_cap, cp + 4u, b.ty);
        xw_put32(out, out_cap, cp + 8u, 0u);
        xw_put32(out, out_cap, cp + 12u, 0u);
    } else {
        xw_put32(out, out_cap, cp, (uint32_t)(int32_t)((int64_t)g.ymin + (int64_t)b.y0));
    }
    xw_put32(out, out_cap, cp + g.chdr - 4u, ds);
    if (ds != csz[q]) {
        uint8_t zh[10];
        zmi_stream_header(1u, level, strategy, zh);
        const uint64_t d0 = cp + g.chdr;
        const uint32_t ad = cadler[q];
        xw_put(out, out_cap, d0, zh[0]);
        xw_put(out, out_cap, d0 + 1u, zh[1]);
#pragma unroll
        for (uint32_t i = 0u; i < 4u; ++i) xw_put(out, out_cap, d0 + ds - 4u + i, ad >> (8u * (3u - i)));
    }
}

// One workgroup of one wave per image: its length and status -- Z_BUF_ERROR where the file crosses out_cap, else the status of the
// least piece that has one, else 0 --, the record of the plan and the channel records, or zeros with the status
__global__ void __launch_bounds__(64) zmi_exr_wwords_kernel(zmi_xw_plan g, const zmi_exr_channel* __restrict__ chs, const uint32_t* __restrict__ cds,
                                                            const uint64_t* __restrict__ cpos, const uint64_t* __restrict__ out_off,
                                                            const uint32_t* __restrict__ bad, const int32_t* __restrict__ st, uint64_t out_cap,
                                                            uint32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                            uint8_t* __restrict__ written, uint8_t* __restrict__ written_ch) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t ql = i * g.nc + g.nc - 1u;
    const uint64_t end = cpos[ql] + g.chdr + cds[ql];
    int32_t s = 0;
    if (end > out_cap) s = ZMI_BUF_ERROR;
    else if (bad[i] != 0xFFFFFFFFu) s = st[bad[i]];
    if (t == 0u) { out_len[i] = s == 0 ? (uint32_t)(end - out_off[i]) : 0u; status[i] = s; }
    if (written) {
        for (uint32_t b = t; b < 88u; b += 64u) {
            uint32_t v = s == 0 ? g.rec[b] : 0u;
            if (s != 0 && b >= 76u && b < 80u) v = ((uint32_t)s >> (8u * (b - 76u))) & 0xFFu;
            written[(uint64_t)i * 88u + b] = (uint8_t)v;
        }
    }
    if (written_ch) {
        const uint8_t* src = (const uint8_t*)chs;
        const uint64_t nb = 24ull * g.n_ch;
        for (uint64_t b = t; b < nb; b += 64u) written_ch[(uint64_t)i * nb + b] = s == 0 ? src[b] : (uint8_t)0u;
    }
}

extern "C" uint32_t zmi_exr_zip_trip(void) { return XW_TRIP; }
extern "C" int zmi_launch_exr_wslice(zmi_xw_slice slice, uint8_t* d_blob, hipStream_t stream) {
    ZMI_LAUNCH(zmi_exr_wslice_kernel, dim3(1), dim3(256), 0, stream, slice, d_blob);
    return 0;
}
extern "C" int zmi_launch_exr_wchunks(zmi_xw_plan plan, const zmi_exr_channel* d_chs, uint32_t* d_csz, uint32_t* d_npc, uint32_t* d_ssz,
                                      uint32_t* d_items, uint32_t* d_cds, uint32_t* d_neff, uint32_t* d_bad, uint64_t* d_run, uint32_t* d_cm,
                                      uint32_t* d_fitems, hipStream_t stream) {
    ZMI_LAUNCH(zmi_exr_wchunks_kernel, dim3(plan.ncc / 256u + 1u), dim3(256), 0, stream, plan, d_chs, d_csz, d_npc, d_ssz, d_items, d_cds, d_neff,
               d_bad, d_run, d_cm, d_fitems);
    return 0;
}
extern "C" int zmi_launch_exr_wpieces(zmi_xw_plan plan, const uint64_t* d_cfirst, const uint64_t* d_soff, const uint32_t* d_csz,
                                      uint32_t group_chunks, uint32_t wpg, uint32_t np, uint64_t* d_poff, uint32_t* d_plen, uint32_t* d_ends,
                                      hipStream_t stream) {
    if (np == 0) return 0;
    ZMI_LAUNCH(zmi_exr_wpieces_kernel, dim3((np + 255u) / 256u), dim3(256), 0, stream, plan, d_cfirst, d_soff, d_csz, group_chunks, wpg, np, d_poff,
               d_plen, d_ends);
    return 0;
}
// bound: the items of the call (the host's count); a fixed grid takes them in turn: a few waves per SIMD
extern "C" int zmi_launch_exr_zip(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off,
                                  const uint64_t* d_item_off, uint64_t bound, const uint64_t* d_soff, uint8_t* d_scan, hipStream_t stream) {
    if (bound == 0) return 0;
    const uint32_t grid = bound > 16384u ? 16384u : (uint32_t)bound;
    ZMI_LAUNCH(zmi_exr_zip_kernel, dim3(grid), dim3(64), 0, stream, plan, d_chs, d_in, d_in_off, d_item_off, d_soff, d_scan);
    return 0;
}
static_assert(XW_P24_TRIP == EXR_P24_TRIP, "zmi_exr_pxr24_trip() states the trip of both PXR24 kernels");
// bound: the items of the call (the host's count)
extern "C" int zmi_launch_exr_pxr24_forward(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off,
                                            const uint64_t* d_fitem_off, uint64_t bound, const uint64_t* d_soff, uint8_t* d_scan,
                                            hipStream_t stream) {
    if (bound == 0) return 0;
    const uint32_t grid = bound > 16384u ? 16384u : (uint32_t)bound;
    ZMI_LAUNCH(zmi_exr_pxr24_forward_kernel, dim3(grid), dim3(64), 0, stream, plan, d_chs, d_in, d_in_off, d_fitem_off, d_soff, d_scan);
    return 0;
}
extern "C" int zmi_launch_exr_wplace(zmi_xw_plan plan, uint32_t first, uint32_t count, const uint64_t* d_cfirst, const uint32_t* d_csz,
                                     const uint32_t* d_olen, const int32_t* d_st, uint64_t* d_run, uint32_t* d_cds, uint64_t* d_cpos,
                                     uint64_t* d_ppos, uint32_t* d_phead, uint64_t* d_out_off, uint32_t* d_bad, hipStream_t stream) {
    ZMI_LAUNCH(zmi_exr_wplace_kernel, dim3(1), dim3(1024), 0, stream, plan, first, count, d_cfirst, d_csz, d_olen, d_st, d_run, d_cds, d_cpos, d_ppos,
               d_phead, d_out_off, d_bad);
    return 0;
}
extern "C" int zmi_launch_exr_gather(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off,
                                     const uint64_t* d_item_off, uint64_t bound, const uint32_t* d_csz, const uint32_t* d_cds,
                                     const uint64_t* d_cpos, uint8_t* d_out, uint64_t out_cap, hipStream_t stream) {
    if (bound == 0) return 0;
    const uint32_t grid = bound > 16384u ? 16384u : (uint32_t)bound;
    ZMI_LAUNCH(zmi_exr_gather_kernel, dim3(grid), dim3(64), 0, stream, plan, d_chs, d_in, d_in_off, d_item_off, d_csz, d_cds, d_cpos, d_out, out_cap);
    return 0;
}
extern "C" int zmi_launch_exr_wframe(zmi_xw_plan plan, const uint8_t* d_hdr, const uint32_t* d_csz, const uint32_t* d_cds, const uint64_t* d_cpos,
                                     const uint32_t* d_cadler, const uint64_t* d_out_off, uint32_t level, uint32_t strategy, uint8_t* d_out,
                                     uint64_t out_cap, hipStream_t stream) {
    ZMI_LAUNCH(zmi_exr_whead_kernel, dim3(plan.n_images), dim3(256), 0, stream, plan, d_hdr, d_out_off, d_out, out_cap);
    ZMI_LAUNCH(zmi_exr_wframe_kernel, dim3((plan.ncc + 255u) / 256u), dim3(256), 0, stream, plan, d_csz, d_cds, d_cpos, d_cadler, d_out_off, level,
               strategy, d_out, out_cap);
    return 0;
}
extern "C" int zmi_launch_exr_wwords(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint32_t* d_cds, const uint64_t* d_cpos,
                                     const uint64_t* d_out_off, const uint32_t* d_bad, const int32_t* d_st, uint64_t out_cap, uint32_t* d_out_len,
                                     int32_t* d_status, zmi_exr_image* d_written, zmi_exr_channel* d_written_channels, hipStream_t stream) {
    ZMI_LAUNCH(zmi_exr_wwords_kernel, dim3(plan.n_images), dim3(64), 0, stream, plan, d_chs, d_cds, d_cpos, d_out_off, d_bad, d_st, out_cap, d_out_len,
               d_status, (uint8_t*)d_written, (uint8_t*)d_written_channels);
    return 0;
}
