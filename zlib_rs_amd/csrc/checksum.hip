// checksum.hip -- Adler-32 and CRC-32 of every shard of a batch, one workgroup per shard.
//
// These are the RFC 1950 / RFC 1952 trailer checksums; the reference computes them in
// zlib-rs/src/adler32.rs:19-47 (BASE 65521, NMAX 5552) + adler32/generic.rs and
// zlib-rs/src/crc32.rs:19-29 + crc32/braid.rs (reflected polynomial 0xEDB88320), fused into
// fill_window / Window::extend.  On the GPU both are restructured around linearity instead of a
// serial fold:
//   Adler-32:  s1 = 1 + sum(b_i),  s2 = n + sum((n - i) * b_i)   (mod 65521)
//              -> every thread takes 16-byte stripes (coalesced), no sequential dependency.
//   CRC-32:    thread t owns one contiguous segment, computes the zero-init raw CRC with a
//              slice-by-16 table in LDS, multiplies it by x^(8 * bytes_after_segment) mod P
//              (the crc32_combine algebra of crc32/combine.rs:26-61 applied per thread) and the
//              workgroup XOR-reduces.  Pre/post conditioning is folded in at the end.
// HBM-bound by construction: 1 byte read per input byte, 4 bytes written per shard.
#include "zmi_device.h"

#define ZMI_ADLER_BASE 65521u

// sum of the four bytes of w, plus acc / sum of byte_i(w) * byte_i(k), plus acc
#ifdef ZMI_EMU
static inline uint32_t zmi_sum4(uint32_t w, uint32_t acc) { return acc + (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24); }
static inline uint32_t zmi_dot4(uint32_t w, uint32_t k, uint32_t acc) {
    for (int i = 0; i < 4; ++i) acc += ((w >> (8 * i)) & 0xFFu) * ((k >> (8 * i)) & 0xFFu);
    return acc;
}
#else
static __device__ __forceinline__ uint32_t zmi_sum4(uint32_t w, uint32_t acc) { return __builtin_amdgcn_sad_u8(w, 0u, acc); }
static __device__ __forceinline__ uint32_t zmi_dot4(uint32_t w, uint32_t k, uint32_t acc) { return __builtin_amdgcn_udot4(w, k, acc, false); }
#endif
#define ZMI_CRC_POLY 0xEDB88320u

// a(x) * b(x) mod P, reflected bit order (bit 31 = x^0)
static __device__ __forceinline__ uint32_t zmi_gf2_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? ZMI_CRC_POLY : 0u);
    }
    return p;
}
// x^(8*nbytes) mod P
static __device__ __forceinline__ uint32_t zmi_gf2_xpow8(uint64_t nbytes) {
    uint32_t r = 0x80000000u;   // x^0
    uint32_t pw = 0x00800000u;  // x^8
    while (nbytes) {
        if (nbytes & 1u) r = zmi_gf2_mulmod(r, pw);
        pw = zmi_gf2_mulmod(pw, pw);
        nbytes >>= 1;
    }
    return r;
}

// the same algebra at compile time, for the two constants of the block scheme below
constexpr uint32_t zmi_cx_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? ZMI_CRC_POLY : 0u);
    }
    return p;
}
constexpr uint32_t zmi_cx_xpow8(uint64_t nbytes) {
    uint32_t r = 0x80000000u, pw = 0x00800000u;
    while (nbytes) {
        if (nbytes & 1u) r = zmi_cx_mulmod(r, pw);
        pw = zmi_cx_mulmod(pw, pw);
        nbytes >>= 1;
    }
    return r;
}
#define CRC_CHUNK 64u                       // bytes a thread takes from a block
#define CRC_BLOCK (256u * CRC_CHUNK)        // bytes the workgroup takes per step
constexpr uint32_t kCrcSkipBlock = zmi_cx_xpow8(CRC_BLOCK - CRC_CHUNK);   // x^(8 * (block - chunk)) mod P
constexpr uint32_t kCrcSkipChunk = zmi_cx_xpow8(CRC_CHUNK);               // x^(8 * chunk) mod P

// v * K mod P through four byte tables of K (multiplication by a constant is linear in v)
static __device__ __forceinline__ uint32_t zmi_crc_mulk(const uint32_t (*kt)[256], uint32_t v) {
    return kt[0][v & 0xFFu] ^ kt[1][(v >> 8) & 0xFFu] ^ kt[2][(v >> 16) & 0xFFu] ^ kt[3][v >> 24];
}

// kind: bit0 = adler32 wanted, bit1 = crc32 wanted.  out_adler/out_crc indexed by shard.
__global__ void __launch_bounds__(256) zmi_checksum_kernel(const uint8_t* __restrict__ data,
                                                           const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ len, uint32_t kind,
                                                           uint32_t* __restrict__ out_adler,
                                                           uint32_t* __restrict__ out_crc) {
    __shared__ uint32_t tab[16][256];
    __shared__ uint32_t kblk[4][256], kchk[4][256], fold[256];
    __shared__ uint32_t red[3][4];
    const uint32_t s = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const uint8_t* src = data + off[s];
    const uint32_t n = len[s];
    const bool aligned = (((uintptr_t)src) & 15u) == 0;

    if (kind & 1u) {
        uint32_t A = 0;
        uint64_t B = 0;   // the weight of byte i is n - i: (n - i0) * (sum of the stripe) - sum(j * b_j) per 16-byte stripe;
                          // a thread's share stays below n * n / 256 * 255 < 2^64, so nothing is reduced inside the loop
        uint32_t i0 = t * 16u;
        // four stripes (four independent 16-byte loads) per trip; byte sums are v_sad_u8 against zero, the weighted sums
        // v_dot4_u32_u8 against the byte offsets: 2 instructions per 4 bytes
        for (; aligned && (uint64_t)i0 + 3u * 4096u + 16u <= n; i0 += 4u * 4096u) {
            uint4 q[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) q[k] = *(const uint4*)(src + i0 + k * 4096u);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t sb = zmi_sum4(q[k].x, zmi_sum4(q[k].y, zmi_sum4(q[k].z, zmi_sum4(q[k].w, 0u))));
                const uint32_t sjb = zmi_dot4(q[k].x, 0x03020100u, zmi_dot4(q[k].y, 0x07060504u,
                                     zmi_dot4(q[k].z, 0x0B0A0908u, zmi_dot4(q[k].w, 0x0F0E0D0Cu, 0u))));
                A += sb;
                B += (uint64_t)(n - i0 - k * 4096u) * sb - sjb;
            }
        }
        for (; i0 < n; i0 += 256u * 16u) {
            uint32_t nv = n - i0;
            zmi_b16 v = zmi_ld16(src + i0, nv, aligned);
            uint32_t sb = 0, sjb = 0;
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) {
                uint32_t b = (v.w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
                sb += b;
                sjb += j * b;
            }
            A += sb;
            // bytes past n were read as zero so they add nothing
            B += (uint64_t)(n - i0) * sb - sjb;
        }
        uint32_t a = A % ZMI_ADLER_BASE;
        uint32_t b = (uint32_t)(B % ZMI_ADLER_BASE);
        a = zmi_wave_sum(a);
        b = zmi_wave_sum(b);
        if (zmi_lane() == 0) { red[0][zmi_wave()] = a % ZMI_ADLER_BASE; red[1][zmi_wave()] = b % ZMI_ADLER_BASE; }
    }
    if (kind & 2u) {
        // slice-by-16 tables: tab[k][b] = CRC of byte b followed by k zero bytes.  One 16-byte step is 16 independent
        // lookups (only the four of the first word wait for the running CRC): one LDS round trip per 16 bytes instead of
        // the four of slice-by-4
        uint32_t c = t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? ZMI_CRC_POLY : 0u);
        tab[0][t] = c;
        __syncthreads();
        for (uint32_t k = 1; k < 16u; ++k) {
            c = (c >> 8) ^ tab[0][c & 0xFFu];
            tab[k][t] = c;
        }
        __syncthreads();
        // Full blocks of 16 KiB: thread t takes the 64 bytes at t * 64 of every block (neighbouring lanes read
        // neighbouring memory; one contiguous 4 KiB segment per thread made every load of a wave touch 64 different
        // lines).  Between two blocks a thread's running value skips the 16 KiB - 64 bytes of the others: a multiplication
        // by the constant x^(8 * 16320), four table reads.  At the end thread 0 folds the 256 values in order
        // (value * x^(8 * 64) + next).
        const uint32_t nfull = aligned ? n / CRC_BLOCK : 0u;
        uint32_t full_raw = 0;
        if (nfull) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                kblk[i][t] = zmi_gf2_mulmod(t << (8u * i), kCrcSkipBlock);
                kchk[i][t] = zmi_gf2_mulmod(t << (8u * i), kCrcSkipChunk);
            }
            __syncthreads();
            uint32_t acc = 0;
            const uint8_t* pch = src + t * CRC_CHUNK;
            for (uint32_t blk = 0; blk < nfull; ++blk, pch += CRC_BLOCK) {
                uint4 q[4];
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) q[k] = *(const uint4*)(pch + 16u * k);
                if (blk) acc = zmi_crc_mulk(kblk, acc);
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    const uint32_t x = acc ^ q[k].x;
                    acc = tab[15][x & 0xFFu] ^ tab[14][(x >> 8) & 0xFFu] ^ tab[13][(x >> 16) & 0xFFu] ^ tab[12][x >> 24] ^
                          tab[11][q[k].y & 0xFFu] ^ tab[10][(q[k].y >> 8) & 0xFFu] ^ tab[9][(q[k].y >> 16) & 0xFFu] ^ tab[8][q[k].y >> 24] ^
                          tab[7][q[k].z & 0xFFu] ^ tab[6][(q[k].z >> 8) & 0xFFu] ^ tab[5][(q[k].z >> 16) & 0xFFu] ^ tab[4][q[k].z >> 24] ^
                          tab[3][q[k].w & 0xFFu] ^ tab[2][(q[k].w >> 8) & 0xFFu] ^ tab[1][(q[k].w >> 16) & 0xFFu] ^ tab[0][q[k].w >> 24];
                }
            }
            fold[t] = acc;
            __syncthreads();
            if (t == 0) {
                uint32_t tot = 0;
                for (uint32_t i = 0; i < 256u; ++i) tot = zmi_crc_mulk(kchk, tot) ^ fold[i];
                full_raw = tot;
            }
        }
        // the rest (everything, for an unaligned shard): one contiguous segment per thread, length multiple of 16
        const uint32_t n0 = nfull * CRC_BLOCK, nt = n - n0;
        const uint8_t* tsrc = src + n0;
        uint32_t seg = ((nt + 255u) / 256u + 15u) & ~15u;
        uint64_t beg = (uint64_t)t * seg;
        uint32_t crc = 0;
        uint64_t after = 0;
        if (beg < nt) {
            uint32_t end = (beg + seg < nt) ? (uint32_t)(beg + seg) : nt;
            after = nt - end;
            for (uint32_t i0 = (uint32_t)beg; i0 < end; i0 += 16u) {
                uint32_t nv = end - i0;
                zmi_b16 v = zmi_ld16(tsrc + i0, nv, aligned);
                if (nv >= 16u) {
                    const uint32_t x = crc ^ v.w[0];
                    uint32_t r = tab[15][x & 0xFFu] ^ tab[14][(x >> 8) & 0xFFu] ^ tab[13][(x >> 16) & 0xFFu] ^ tab[12][x >> 24];
#pragma unroll
                    for (int q = 1; q < 4; ++q) {
                        const uint32_t y = v.w[q];
                        r ^= tab[15 - 4 * q][y & 0xFFu] ^ tab[14 - 4 * q][(y >> 8) & 0xFFu] ^ tab[13 - 4 * q][(y >> 16) & 0xFFu] ^
                             tab[12 - 4 * q][y >> 24];
                    }
                    crc = r;
                } else {
                    for (uint32_t j = 0; j < nv; ++j) {
                        uint32_t b = (v.w[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
                        crc = tab[0][(crc ^ b) & 0xFFu] ^ (crc >> 8);
                    }
                }
            }
            crc = zmi_gf2_mulmod(crc, zmi_gf2_xpow8(after));
        }
        if (t == 0 && nfull) crc ^= zmi_gf2_mulmod(full_raw, zmi_gf2_xpow8(nt));   // the full blocks, moved in front of the rest
        // xor-reduce
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) crc ^= __shfl_xor(crc, d);
        if (zmi_lane() == 0) red[2][zmi_wave()] = crc;
    }
    __syncthreads();
    if (t == 0) {
        if (kind & 1u) {
            uint32_t a = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) % ZMI_ADLER_BASE;
            uint32_t b = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) % ZMI_ADLER_BASE;
            uint32_t s1 = (1u + a) % ZMI_ADLER_BASE;
            uint32_t s2 = (n % ZMI_ADLER_BASE + b) % ZMI_ADLER_BASE;
            out_adler[s] = (s2 << 16) | s1;
        }
        if (kind & 2u) {
            uint32_t raw = red[2][0] ^ red[2][1] ^ red[2][2] ^ red[2][3];
            // init 0xFFFFFFFF travels through n bytes, then final inversion
            uint32_t init = zmi_gf2_mulmod(0xFFFFFFFFu, zmi_gf2_xpow8(n));
            out_crc[s] = raw ^ init ^ 0xFFFFFFFFu;
        }
    }
}

extern "C" int zmi_launch_checksum(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                                   uint32_t n_shards, uint32_t kind, uint32_t* d_adler, uint32_t* d_crc,
                                   hipStream_t stream) {
    if (n_shards == 0 || (kind & 3u) == 0) return 0;
    ZMI_LAUNCH(zmi_checksum_kernel, dim3(n_shards), dim3(256), 0, stream, d_data, d_off, d_len, kind, d_adler, d_crc);
    return 0;
}

// ---- checksum combine: the check value of a concatenation from the pieces' (check, raw length) pairs -----------------------
// The reference stitches the trailer of its parallel-deflate recipe serially: crc32_combine (crc32/combine.rs:3-13) and
// adler32_combine (adler32.rs:58), one call per piece.  Both are associative operators on (check, length) pairs:
//   CRC-32:   (c1, l1) o (c2, l2) = (c1 * x^(8 * l2) mod P  xor  c2,  l1 + l2)
//   Adler-32: (a1, l1) o (a2, l2) = (adler32_combine(a1, a2, l2 mod 65521),  l1 + l2)
// so the device reduces them in a tree: every lane folds a run of consecutive entries, the wave folds its 64 lanes in order
// with an xor butterfly (the lower partner combines mine o theirs, the upper theirs o mine), wave 0 folds the four wave results,
// and a second launch folds the per-workgroup results when there were several.  x^(8 * l) is the product of x^(8 * 2^k) over the
// set bits of l (a table of 64 powers, built at compile time): one multiplication per piece for power-of-two piece sizes.
// An entry of length 0 is the identity whatever its check field holds (the multi-GPU tables are padded with zeros).
#define ZMI_COMBINE_T 256u
#define ZMI_COMBINE_PER_LANE 16u
struct zmi_xpow_tab { uint32_t v[64]; };
constexpr zmi_xpow_tab zmi_cx_xpow_tab() {
    zmi_xpow_tab t{};
    uint32_t p = 0x00800000u;   // x^8
    for (int k = 0; k < 64; ++k) { t.v[k] = p; p = zmi_cx_mulmod(p, p); }
    return t;
}
constexpr zmi_xpow_tab kXpowTab = zmi_cx_xpow_tab();

static __device__ __forceinline__ uint32_t zmi_adler_combine_dev(uint32_t a1, uint32_t a2, uint64_t len2) {
    const uint32_t rem = (uint32_t)(len2 % ZMI_ADLER_BASE);
    uint32_t s1 = a1 & 0xFFFFu;
    uint32_t s2 = (uint32_t)(((uint64_t)rem * s1) % ZMI_ADLER_BASE);
    s1 += (a2 & 0xFFFFu) + ZMI_ADLER_BASE - 1u;
    s2 += ((a1 >> 16) & 0xFFFFu) + ((a2 >> 16) & 0xFFFFu) + ZMI_ADLER_BASE - rem;
    if (s1 >= ZMI_ADLER_BASE) s1 -= ZMI_ADLER_BASE;
    if (s1 >= ZMI_ADLER_BASE) s1 -= ZMI_ADLER_BASE;
    if (s2 >= 2u * ZMI_ADLER_BASE) s2 -= 2u * ZMI_ADLER_BASE;
    if (s2 >= ZMI_ADLER_BASE) s2 -= ZMI_ADLER_BASE;
    return (s2 << 16) | s1;
}
// (c1, l1) o (c2, l2) in place of (c1, l1); pw = the x^(8 * 2^k) table
static __device__ __forceinline__ void zmi_combine_pair(bool adler, const uint32_t* pw, uint32_t& c1, uint64_t& l1, uint32_t c2,
                                                        uint64_t l2) {
    if (l2 == 0) return;
    if (l1 == 0) { c1 = c2; l1 = l2; return; }
    if (adler) {
        c1 = zmi_adler_combine_dev(c1, c2, l2);
    } else {
        for (uint64_t b = l2; b; b &= b - 1u) c1 = zmi_gf2_mulmod(c1, pw[__builtin_ctzll(b)]);
        c1 ^= c2;
    }
    l1 += l2;
}

// One workgroup folds the logical entries [blockIdx.x * per_block, + per_block) of n.  Logical entry g is table entry
// (g % world) * n_local + g / world (the rank-major all-gathered tables; world 1 = plain order).  Lengths come from len32
// (the tables) or, in the second pass over the workgroups' results, from len64.  out_check / out_len[blockIdx.x] = the fold.
__global__ void __launch_bounds__(ZMI_COMBINE_T) zmi_combine_kernel(const uint32_t* __restrict__ check, const uint32_t* __restrict__ len32,
                                                                   const uint64_t* __restrict__ len64, uint32_t n, uint32_t world,
                                                                   uint32_t n_local, uint32_t per_block, uint32_t adler,
                                                                   uint32_t* __restrict__ out_check, uint64_t* __restrict__ out_len) {
    __shared__ uint32_t pw[64];
    __shared__ uint32_t wc[ZMI_COMBINE_T / 64u];
    __shared__ uint64_t wl[ZMI_COMBINE_T / 64u];
    const uint32_t t = threadIdx.x;
    if (t < 64u) pw[t] = kXpowTab.v[t];
    __syncthreads();
    const bool ad = adler != 0u;
    const uint64_t b0 = (uint64_t)blockIdx.x * per_block;
    const uint64_t b1 = b0 + per_block < n ? b0 + per_block : n;
    const uint32_t per_lane = (per_block + ZMI_COMBINE_T - 1u) / ZMI_COMBINE_T;
    uint32_t c = ad ? 1u : 0u;
    uint64_t l = 0;
    for (uint64_t g = b0 + (uint64_t)t * per_lane, ge = g + per_lane; g < ge && g < b1; ++g) {
        const uint64_t idx = world == 1u ? g : (g % world) * n_local + g / world;
        zmi_combine_pair(ad, pw, c, l, check[idx], len64 ? len64[idx] : (uint64_t)len32[idx]);
    }
    // ordered butterfly: after step d every lane holds the fold of its aligned run of 2d lanes
    const uint32_t lane = zmi_lane();
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t oc = __shfl_xor(c, (int)d);
        const uint32_t olo = __shfl_xor((uint32_t)l, (int)d), ohi = __shfl_xor((uint32_t)(l >> 32), (int)d);
        const uint64_t ol = ((uint64_t)ohi << 32) | olo;
        if (lane & d) {
            uint32_t c2 = oc;
            uint64_t l2 = ol;
            zmi_combine_pair(ad, pw, c2, l2, c, l);
            c = c2;
            l = l2;
        } else {
            zmi_combine_pair(ad, pw, c, l, oc, ol);
        }
    }
    if (lane == 0) { wc[zmi_wave()] = c; wl[zmi_wave()] = l; }
    __syncthreads();
    if (t == 0) {
        for (uint32_t w = 1; w < ZMI_COMBINE_T / 64u; ++w) zmi_combine_pair(ad, pw, c, l, wc[w], wl[w]);
        out_check[blockIdx.x] = c;
        out_len[blockIdx.x] = l;
    }
}

// d_partial: room for zmi_combine_partials(n) check words and as many u64 lengths (NULL when that is 1)
extern "C" uint32_t zmi_combine_partials(uint32_t n) {
    const uint32_t per_block = ZMI_COMBINE_T * ZMI_COMBINE_PER_LANE;
    return n <= per_block ? 1u : (uint32_t)(((uint64_t)n + per_block - 1u) / per_block);
}
extern "C" int zmi_launch_checksum_combine(const uint32_t* d_check, const uint32_t* d_len, uint32_t n, uint32_t world, uint32_t n_local,
                                           uint32_t adler, uint32_t* d_pc, uint64_t* d_pl, uint32_t* d_out_check, uint64_t* d_out_len,
                                           hipStream_t stream) {
    const uint32_t nb = zmi_combine_partials(n);
    if (nb == 1u) {
        ZMI_LAUNCH(zmi_combine_kernel, dim3(1), dim3(ZMI_COMBINE_T), 0, stream, d_check, d_len, (const uint64_t*)nullptr, n, world, n_local,
                   n, adler, d_out_check, d_out_len);
        return 0;
    }
    ZMI_LAUNCH(zmi_combine_kernel, dim3(nb), dim3(ZMI_COMBINE_T), 0, stream, d_check, d_len, (const uint64_t*)nullptr, n, world, n_local,
               ZMI_COMBINE_T * ZMI_COMBINE_PER_LANE, adler, d_pc, d_pl);
    ZMI_LAUNCH(zmi_combine_kernel, dim3(1), dim3(ZMI_COMBINE_T), 0, stream, (const uint32_t*)d_pc, (const uint32_t*)nullptr,
               (const uint64_t*)d_pl, nb, 1u, nb, nb, adler, d_out_check, d_out_len);
    return 0;
}

// ---- the CRC-32 of every entry of a piece table (zmi_zip_write_dev; adler != 0: the Adler-32, zmi_png_encode_dev) -------------------------
// Segment e < *n_live (a device word, at most the n the launch covers) is the pieces [first[e], first[e + 1]) of the (check, len)
// tables; out[e] = their fold, a copy of the word where the segment
// is one piece.  One thread per segment folds up to ZMI_SEG_SERIAL pieces in order -- an archive of small files is all such segments,
// and a wave per segment would be 64 lanes for one multiplication.  A longer segment (a 1 GiB entry in 1 MiB pieces: 1024 dependent
// combines, ~0.1 ms on one lane) is folded by the whole wave afterwards, one such segment at a time: every lane a run of consecutive
// pieces, then the ordered butterfly of zmi_combine_kernel.
#define ZMI_SEG_SERIAL 64u
__global__ void __launch_bounds__(256) zmi_combine_segments_kernel(const uint32_t* __restrict__ check, const uint32_t* __restrict__ len,
                                                                  const uint64_t* __restrict__ first, const uint32_t* __restrict__ n_live,
                                                                  uint32_t adler, uint32_t* __restrict__ out) {
    __shared__ uint32_t pw[64];
    const uint32_t t = threadIdx.x;
    if (t < 64u) pw[t] = kXpowTab.v[t];
    __syncthreads();
    const bool ad = adler != 0u;
    const uint64_t gi = (uint64_t)blockIdx.x * 256u + t;
    const bool live = gi < *n_live;
    const uint64_t p0 = live ? first[gi] : 0ull, cnt = live ? first[gi + 1u] - p0 : 0ull;
    if (live && cnt <= ZMI_SEG_SERIAL) {
        uint32_t c = ad ? 1u : 0u;
        uint64_t l = 0;
        for (uint64_t p = p0; p < p0 + cnt; ++p) zmi_combine_pair(ad, pw, c, l, check[p], (uint64_t)len[p]);
        out[gi] = c;
    }
    const uint32_t lane = zmi_lane();
    for (uint64_t big = __ballot(cnt > ZMI_SEG_SERIAL); big; big &= big - 1u) {   // (the same trips in every lane of the wave)
        const int src = __ffsll((unsigned long long)big) - 1;
        const uint64_t q0 = ((uint64_t)__shfl((uint32_t)(p0 >> 32), src) << 32) | __shfl((uint32_t)p0, src);
        const uint64_t qn = ((uint64_t)__shfl((uint32_t)(cnt >> 32), src) << 32) | __shfl((uint32_t)cnt, src);
        const uint64_t per = (qn + 63u) / 64u;
        uint32_t c = ad ? 1u : 0u;
        uint64_t l = 0;
        for (uint64_t p = lane * per; p < (lane + 1u) * per && p < qn; ++p) zmi_combine_pair(ad, pw, c, l, check[q0 + p], (uint64_t)len[q0 + p]);
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t oc = __shfl_xor(c, (int)d);
            const uint32_t olo = __shfl_xor((uint32_t)l, (int)d), ohi = __shfl_xor((uint32_t)(l >> 32), (int)d);
            const uint64_t ol = ((uint64_t)ohi << 32) | olo;
            if (lane & d) {
                uint32_t c2 = oc;
                uint64_t l2 = ol;
                zmi_combine_pair(ad, pw, c2, l2, c, l);
                c = c2;
                l = l2;
            } else {
                zmi_combine_pair(ad, pw, c, l, oc, ol);
            }
        }
        if (lane == 0u) out[gi - lane + (uint32_t)src] = c;   // (lane 0's gi is the wave's first segment)
    }
}
extern "C" int zmi_launch_combine_segments(const uint32_t* d_check, const uint32_t* d_len, const uint64_t* d_first, uint32_t n,
                                           const uint32_t* d_n_live, uint32_t* d_out, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_combine_segments_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_check, d_len, d_first, d_n_live, 0u, d_out);
    return 0;
}
// the same fold of Adler-32 values (zmi_png_encode_dev: the scanlines of an image from its pieces'); a segment without pieces gives 1
extern "C" int zmi_launch_combine_segments_adler(const uint32_t* d_check, const uint32_t* d_len, const uint64_t* d_first, uint32_t n,
                                                 const uint32_t* d_n_live, uint32_t* d_out, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_combine_segments_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_check, d_len, d_first, d_n_live, 1u, d_out);
    return 0;
}
