// zmi_api.hip -- host side of the batch C ABI declared in include/zmi355.h.
//
// Orchestrates the kernel pipeline on the caller's HIP stream:
//   deflate:  [checksum] -> lz77 (match per position) -> encode (parse + Huffman + bit pack)
//   inflate:  inflate -> checksum of the produced bytes -> verify against the trailer
// Device scratch (4 B per input byte for the match/token array) is owned by the context and the
// batch is cut into groups that fit it.  No CPU fallback exists: without a HIP device every entry
// point fails with ZMI_E_NODEVICE.
#include "zmi_kernels.h"
#include "zmi_scratch.h"
#include "../../include/zmi355.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <atomic>
#include <algorithm>
#include <string>
#include <vector>

static thread_local std::string g_err;
static int zmi_fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[256];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}
// Tuning overrides (ZMI_CHAIN, ZMI_BLOCK_SPAN, ZMI_HOST_CHUNK ...) exist for the tests and the probe tools.  They are read
// only in a process that was started with ZMI_TUNING set: checked once, so a product process never calls getenv() on its
// hot path and its behaviour does not depend on whatever else is in the environment.
static const char* zmi_tune(const char* name) {
    static const bool enabled = getenv("ZMI_TUNING") != nullptr;
    return enabled ? getenv(name) : nullptr;
}
#define ZMI_HIP(call)                                              \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return zmi_fail(ZMI_E_HIP, #call, e_); \
    } while (0)

// Every entry point runs on the context's device and leaves the calling thread's current device as it found it (a
// process that drives several GPUs -- one torch process with libz_mi355 loaded -- must not have its device switched
// under it).
struct zmi_dev_guard {
    int prev = -1;
    bool switched = false, ok = true;
    explicit zmi_dev_guard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; switched = ok && prev >= 0; }
    }
    ~zmi_dev_guard() { if (switched) (void)hipSetDevice(prev); }
};
#define ZMI_ON_DEVICE(c)                                         \
    zmi_dev_guard dev_guard_((c)->device);                       \
    if (!dev_guard_.ok) return zmi_fail(ZMI_E_HIP, "hipSetDevice")

struct zmi_buf {
    void* p = nullptr;
    size_t cap = 0;
};

struct zmi_timer {
    hipEvent_t a, b;
    int kernel;
};
enum { ZMI_K_CHECKSUM = 0, ZMI_K_LZ77 = 1, ZMI_K_ENCODE = 2, ZMI_K_INFLATE = 3, ZMI_K_VERIFY = 4, ZMI_K_PARSE = 5, ZMI_K_RESOLVE = 6, ZMI_K_PACK = 7 };

#define ZMI_HB_SLOTS 3   // host-buffer pipelines: chunks in flight (staging in, on the device, staging out)
struct zmi_ctx {
    bool timing = false;
    std::vector<zmi_timer> timers;
    int device = 0;
    uint64_t scratch_limit = 8ull << 30;
    zmi_buf match;    // u32 per position of the current group
    zmi_buf sums;     // adler[n] crc[n]
    zmi_buf pieces;   // per shard x piece compressed length
    zmi_buf inf_tmp;  // inflate: the per-stream tables of one launch (zmi_inf_tables_of states the layout; callers get zmi_inf_scratch)
    zmi_buf inf_bm;   // inflate: 1 bit per output byte of the batch (where back-references start)
    zmi_buf inf_ptr;  // inflate of few streams: 4 B per output byte, the pointers of the jump resolve (resolve_jump.hip)
    zmi_buf st_in, st_out, st_meta;  // zmi_inflate_resume: staging of one host stream (kept across calls)
    zmi_buf sp_out;                  // zmi_inflate_split: the segments' decode regions
    zmi_buf st_scan;                 // zmi_inflate_blocks: the block scan's counter and list
    zmi_buf st_pin[2];               // zmi_d2h: two pinned 4 MiB pieces the decoded bytes of a single stream leave through
    hipEvent_t st_pin_ev[2]{};
    bool st_pin_ev_live = false;
    // host-buffer batches (zmi_deflate_batch): two slots cycle through copy-in / kernels / copy-out on three streams
    struct hb_slot { zmi_buf in, out, meta; hipEvent_t in_done, k_done, out_done; } hb[ZMI_HB_SLOTS];
    zmi_buf hb_slab[ZMI_HB_SLOTS];                              // device: the chunk's compressed streams packed densely (what travels back)
    zmi_buf hb_pin_in[ZMI_HB_SLOTS], hb_pin_out[ZMI_HB_SLOTS], hb_pin_meta[ZMI_HB_SLOTS];   // pinned host staging of the two slots
    hipStream_t hs_in = nullptr, hs_k = nullptr, hs_out = nullptr, hs_slab = nullptr;
    bool hb_live = false;
    uint64_t pinned_limit = 10ull << 30;   // host-buffer pipelines: pinned staging this context may hold (chunk sizes follow it; env ZMI_PINNED_MB)
    std::atomic<int> hb_out_tight{-1};     // zmi_inflate_batch: did the last chunk decoded fill most of its capacity?  (-1: nothing decoded yet)
    uint32_t last_codes_used = 0;    // zmi_inflate_resume: table entries of the most recent dynamic block of the last call (inflateCodesUsed)
    uint64_t inflate_out_limit = 0;  // zmi_ctx_set_inflate_out_limit, written nowhere else: output bytes an inflate call that does not size
                                     // its own scratch (zmi_inf_req::out_limit = 0) may cover; 0 = scratch_limit
    uint32_t inf_mw_max = 512u;      // inflate launches of up to this many streams give every stream a 16-wave workgroup (inflate.hip)
    hipStream_t host_stream = nullptr;  // zmi_ctx_set_stream: where the host-buffer wrappers copy and launch
    hipStream_t side = nullptr;         // deflate: the wrapper checksums run here, beside the match search (zmi_deflate_impl)
    hipEvent_t ev_fork{}, ev_join{};
    zmi_buf sd_meta, sd_slots;          // zmi_deflate_stream_dev, the BGZF calls: per-piece tables / one launch group's output slots
    zmi_buf comb;                       // zmi_checksum_combine_dev: the per-workgroup partial folds
    zmi_buf si_meta, si_work, si_seg;   // zmi_inflate_stream_dev: per-piece tables / one launch group's regions; find_cuts' segment table
    zmi_buf si_scan;                    // zmi_stream_find_blocks_dev: one window's survivor slots and validated list
    zmi_buf mm_scan, mm_meta;           // zmi_gzip_find_members_dev: segment counts and offsets; zmi_inflate_members_dev: its tables
    zmi_buf pk;                         // zmi_inflate_batch_packed_dev: size[n] cap[n] (the size pass's result, the planned capacity table)
    zmi_buf zip_dir, zip_sel;           // zmi_zip_directory_dev: four words, the chain positions, four words per segment; zmi_zip_inflate_dev: the slots' tables
    zmi_buf tiff_dir;                   // zmi_tiff_directory_dev: the positions of the listed IFDs
    zmi_buf tiff;                       // zmi_tiff_read_dev: the slots' tables | the still-predicted segments
    zmi_buf tiff_w;                     // zmi_tiff_write_dev: the piece table | the predicted segments
    zmi_buf exr;                        // zmi_exr_read_dev: the slots', chunks' and blocks' tables | the inflated chunks
    zmi_buf png;                        // zmi_png_decode_dev: the slots' tables | the gathered IDAT streams | the filtered scanlines
    zmi_buf dict;                       // the shared-dictionary batch calls: layout words and DICTID | deflate image | inflate image (zmi_sd_*)
};

static int zmi_reserve(zmi_buf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = (bytes + 0xFFFFFull) & ~(size_t)0xFFFFFull;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return zmi_fail(ZMI_E_NOMEM, "hipMalloc(scratch)", e);
    b.cap = want;
    return 0;
}

// A call's tables in one context buffer: `layout` (zmi_scratch.h: a function of a carver that takes every table once and returns the
// carver's end) sizes the reservation, then yields the pointers.  The capacity the emulator build holds the takes to is the size
// that was asked for, not what zmi_reserve rounded it up to.
template <class L> static int zmi_carve(zmi_buf& b, L&& layout) {
    const size_t bytes = layout(zmi_carver());
    int rc = zmi_reserve(b, bytes);
    if (rc) return rc;
    layout(zmi_carver(b.p, bytes));
    return 0;
}

// ---- the argument checks the container calls share (the texts are part of the interface: tests and callers match on them) ----
static int zmi_check_out_align(uint32_t out_align) {
    if (out_align == 0u || out_align > 4096u || (out_align & (out_align - 1u)) != 0u)
        return zmi_fail(ZMI_E_ARG, "out_align must be a power of two, 1 .. 4096");
    return ZMI_E_OK;
}
static int zmi_check_level_strategy(int& level, int strategy) {   // (-1: the default level, 6)
    if (level == -1) level = 6;
    if (level < 0 || level > 9) return zmi_fail(ZMI_E_ARG, "level must be -1..9");
    if (strategy < 0 || strategy > 4) return zmi_fail(ZMI_E_ARG, "strategy must be 0..4");
    return ZMI_E_OK;
}
static int zmi_check_piece_bytes(uint32_t piece_bytes) {
    if (piece_bytes == 0 || piece_bytes > (1u << 30)) return zmi_fail(ZMI_E_ARG, "piece_bytes must be 1 .. 2^30");
    return ZMI_E_OK;
}
// The readers' empty selection (ZIP, PNG, TIFF, EXR): nothing is read, d_out_off[0] = 0 is the whole result and the call is *done;
// any other selection needs the result arrays.
static int zmi_empty_selection(uint32_t n_sel, uint64_t* d_out_off, const void* d_out_len, const void* d_status, const void* d_detail,
                               hipStream_t stream, bool* done) {
    *done = n_sel == 0;
    if (n_sel == 0) {
        ZMI_HIP(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), stream));
        return ZMI_E_OK;
    }
    if (!d_out_len || !d_status || !d_detail) return zmi_fail(ZMI_E_ARG, "d_out_len, d_status and d_detail are required");
    return ZMI_E_OK;
}

extern "C" const char* zmi_version(void) { return "zmi355 0.1.0 (gfx950; zlib ABI 1.3.0-zlib-rs-0.6.7 compatible)"; }
extern "C" const char* zmi_last_error(void) { return g_err.c_str(); }
// the other translation units of this library (exchange.hip) report through the same thread-local message
extern "C" void zmi_set_last_error(const char* what) { g_err = what ? what : ""; }

extern "C" int zmi_ctx_create(zmi_ctx** out, int device) {
    if (!out) return zmi_fail(ZMI_E_ARG, "zmi_ctx_create: null out pointer");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return zmi_fail(ZMI_E_NODEVICE, "no HIP device (this library has no CPU path)", e);
    if (device < 0 || device >= ndev) return zmi_fail(ZMI_E_ARG, "zmi_ctx_create: device index out of range");
    zmi_ctx* c = new zmi_ctx();
    c->device = device;
    const char* env = getenv("ZMI_SCRATCH_MB");
    if (env && atoll(env) > 0) c->scratch_limit = (uint64_t)atoll(env) << 20;
    env = getenv("ZMI_PINNED_MB");
    if (env && atoll(env) >= 64) c->pinned_limit = (uint64_t)atoll(env) << 20;
    *out = c;
    return ZMI_E_OK;
}

extern "C" int zmi_ctx_destroy(zmi_ctx* c) {
    if (!c) return ZMI_E_OK;
    zmi_dev_guard dev_guard_(c->device);
    if (c->match.p) (void)hipFree(c->match.p);
    if (c->sums.p) (void)hipFree(c->sums.p);
    if (c->pieces.p) (void)hipFree(c->pieces.p);
    if (c->inf_tmp.p) (void)hipFree(c->inf_tmp.p);
    if (c->inf_bm.p) (void)hipFree(c->inf_bm.p);
    if (c->inf_ptr.p) (void)hipFree(c->inf_ptr.p);
    if (c->st_in.p) (void)hipFree(c->st_in.p);
    if (c->st_out.p) (void)hipFree(c->st_out.p);
    if (c->st_meta.p) (void)hipFree(c->st_meta.p);
    if (c->side) { (void)hipStreamDestroy(c->side); (void)hipEventDestroy(c->ev_fork); (void)hipEventDestroy(c->ev_join); }
    if (c->sp_out.p) (void)hipFree(c->sp_out.p);
    if (c->st_scan.p) (void)hipFree(c->st_scan.p);
    if (c->sd_meta.p) (void)hipFree(c->sd_meta.p);
    if (c->sd_slots.p) (void)hipFree(c->sd_slots.p);
    if (c->comb.p) (void)hipFree(c->comb.p);
    if (c->si_meta.p) (void)hipFree(c->si_meta.p);
    if (c->si_work.p) (void)hipFree(c->si_work.p);
    if (c->si_seg.p) (void)hipFree(c->si_seg.p);
    if (c->si_scan.p) (void)hipFree(c->si_scan.p);
    if (c->dict.p) (void)hipFree(c->dict.p);
    if (c->pk.p) (void)hipFree(c->pk.p);
    if (c->zip_dir.p) (void)hipFree(c->zip_dir.p);
    if (c->zip_sel.p) (void)hipFree(c->zip_sel.p);
    if (c->png.p) (void)hipFree(c->png.p);
    if (c->tiff.p) (void)hipFree(c->tiff.p);
    if (c->tiff_dir.p) (void)hipFree(c->tiff_dir.p);
    if (c->tiff_w.p) (void)hipFree(c->tiff_w.p);
    if (c->exr.p) (void)hipFree(c->exr.p);
    if (c->mm_scan.p) (void)hipFree(c->mm_scan.p);
    if (c->mm_meta.p) (void)hipFree(c->mm_meta.p);
    for (int k = 0; k < 2; ++k) if (c->st_pin[k].p) (void)hipHostFree(c->st_pin[k].p);
    if (c->st_pin_ev_live) { (void)hipEventDestroy(c->st_pin_ev[0]); (void)hipEventDestroy(c->st_pin_ev[1]); }
    if (c->hb_live) {
        for (auto& sl : c->hb) {
            if (sl.in.p) (void)hipFree(sl.in.p);
            if (sl.out.p) (void)hipFree(sl.out.p);
            if (sl.meta.p) (void)hipFree(sl.meta.p);
            (void)hipEventDestroy(sl.in_done); (void)hipEventDestroy(sl.k_done); (void)hipEventDestroy(sl.out_done);
        }
        for (int k = 0; k < ZMI_HB_SLOTS; ++k) {
            if (c->hb_slab[k].p) (void)hipFree(c->hb_slab[k].p);
            if (c->hb_pin_in[k].p) (void)hipHostFree(c->hb_pin_in[k].p);
            if (c->hb_pin_out[k].p) (void)hipHostFree(c->hb_pin_out[k].p);
            if (c->hb_pin_meta[k].p) (void)hipHostFree(c->hb_pin_meta[k].p);
        }
        (void)hipStreamDestroy(c->hs_in); (void)hipStreamDestroy(c->hs_k); (void)hipStreamDestroy(c->hs_out); if (c->hs_slab) (void)hipStreamDestroy(c->hs_slab);
    }
    delete c;
    return ZMI_E_OK;
}

// per-kernel HIP-event timing (used by bench.py for the roofline line; off by default)
struct zmi_scope_timer {
    zmi_ctx* c;
    hipStream_t st;
    zmi_timer t;
    bool on;
    zmi_scope_timer(zmi_ctx* c_, int kernel, hipStream_t st_) : c(c_), st(st_), on(c_->timing) {
        if (!on) return;
        t.kernel = kernel;
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(t.a, st);
    }
    ~zmi_scope_timer() {
        if (!on) return;
        (void)hipEventRecord(t.b, st);
        c->timers.push_back(t);
    }
};

extern "C" int zmi_ctx_device(const zmi_ctx* c) { return c ? c->device : -1; }

// The single-stream host wrappers (zmi_inflate_resume) copy and launch on this stream and wait for it alone -- a caller
// that gives every context its own non-blocking stream can drive several contexts from several threads without one
// call stalling the device for the others (the stream ABI does, zlib_abi.hip).  Default: the null stream.
extern "C" int zmi_ctx_set_stream(zmi_ctx* c, void* stream) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    c->host_stream = (hipStream_t)stream;
    return ZMI_E_OK;
}

// decode-table entries (literal / length + distance; roots 9 / 8, exact-fit sub-tables) the device built for the most recent
// dynamic block met by zmi_inflate_resume calls on this context; 0 before the first one.  What inflateCodesUsed reports.
extern "C" int zmi_ctx_last_codes_used(zmi_ctx* c, uint32_t* entries) {
    if (!c || !entries) return zmi_fail(ZMI_E_ARG, "null argument");
    *entries = c->last_codes_used;
    return ZMI_E_OK;
}
extern "C" int zmi_ctx_reset_codes_used(zmi_ctx* c) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    c->last_codes_used = 0;
    return ZMI_E_OK;
}

extern "C" int zmi_ctx_set_timing(zmi_ctx* c, int on) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    c->timing = on != 0;
    return ZMI_E_OK;
}

// sums[k] = total milliseconds of kernel k since the last call, counts[k] = launches (k < 8)
extern "C" int zmi_ctx_get_timing(zmi_ctx* c, double* sums, uint32_t* counts) {
    if (!c || !sums || !counts) return zmi_fail(ZMI_E_ARG, "null argument");
    for (int k = 0; k < 8; ++k) { sums[k] = 0; counts[k] = 0; }
    for (zmi_timer& t : c->timers) {
        (void)hipEventSynchronize(t.b);
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess && t.kernel >= 0 && t.kernel < 8) {
            sums[t.kernel] += ms;
            counts[t.kernel]++;
        }
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    c->timers.clear();
    return ZMI_E_OK;
}

extern "C" int zmi_ctx_set_scratch_limit(zmi_ctx* c, uint64_t bytes) {
    if (!c || bytes < (64ull << 20)) return zmi_fail(ZMI_E_ARG, "scratch limit must be >= 64 MiB");
    c->scratch_limit = bytes;
    return ZMI_E_OK;
}

extern "C" int zmi_ctx_set_inflate_out_limit(zmi_ctx* c, uint64_t bytes) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    c->inflate_out_limit = bytes < (1ull << 20) ? (1ull << 20) : bytes;
    return ZMI_E_OK;
}

extern "C" uint64_t zmi_deflate_bound(uint64_t n, int wrap) {
    // zlib-rs/src/deflate.rs:2975-2991 (compress_bound_help) with wrap overhead 0 / 6 / 18
    uint64_t w = wrap == ZMI_WRAP_ZLIB ? 6u : (wrap == ZMI_WRAP_GZIP ? 18u : 0u);
    uint64_t b = n + (n == 0) + (n < 9) + ((n + 7) >> 3) + 3 + w;
    // this engine's own worst case is a run of stored blocks (5 bytes per 32 KiB) -- far below the above
    return (b + 15) & ~15ull;
}

extern "C" uint64_t zmi_deflate_dict_bound(uint64_t n, int wrap) {
    // ... and the DICTID behind the zlib header (deflate.rs:1572-1601)
    uint64_t w = wrap == ZMI_WRAP_ZLIB ? 10u : (wrap == ZMI_WRAP_GZIP ? 18u : 0u);
    uint64_t b = n + (n == 0) + (n < 9) + ((n + 7) >> 3) + 3 + w;
    return (b + 15) & ~15ull;
}

// One preset dictionary for every shard / stream of a batch call (zmi_deflate_batch_shared_dict_dev,
// zmi_inflate_batch_shared_dict_dev): what the kernels read lives in the context's `dict` scratch, built on the caller's stream by
// zmi_launch_dict_image and the checksum kernel -- no value of it passes through the host.
#define ZMI_SD_LAY_OFF 0u        // u64: 0            } the one-entry layout the checksum kernel reads the dictionary through
#define ZMI_SD_LAY_LEN 8u        // u32: dict_len     }
#define ZMI_SD_DICTID 12u        // u32: Adler-32 of all dict_len bytes
#define ZMI_SD_DEF_IMG 64u       // deflate: the tail the match search can reach, <= 27 648 bytes (zmi_lz77_dict_image_len)
#define ZMI_SD_INF_IMG 32832u    // inflate: the last <= 32 768 bytes, ending at a multiple of 1 KiB, zeros in front and 32 behind
#define ZMI_SD_BYTES (ZMI_SD_INF_IMG + 32768u + 64u)
struct zmi_sd_deflate {
    const uint8_t* img;       // null / 0: no history (a dictionary shorter than 16 bytes, Z_HUFFMAN_ONLY)
    uint32_t img_len;
    const uint32_t* dictid;   // device word (zlib wrapper only)
};
struct zmi_sd_inflate {
    const uint8_t* img;
    uint32_t hist;            // min(dict_len, 32768)
    const uint32_t* dictid;
};
static int zmi_sd_prepare(zmi_ctx* c, const void* d_dict, uint32_t dict_len, bool inflate, bool want_id, hipStream_t stream,
                          uint32_t lead, uint32_t take, uint32_t pad) {
    int rc = zmi_reserve(c->dict, ZMI_SD_BYTES);
    if (rc) return rc;
    uint8_t* base = (uint8_t*)c->dict.p;
    int lrc = zmi_launch_dict_image((const uint8_t*)d_dict, dict_len, base + (inflate ? ZMI_SD_INF_IMG : ZMI_SD_DEF_IMG), lead, take, pad,
                                    (uint64_t*)(base + ZMI_SD_LAY_OFF), (uint32_t*)(base + ZMI_SD_LAY_LEN), stream);
    if (lrc) return zmi_fail(ZMI_E_ARG, "dictionary image layout");
    if (want_id) {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_checksum((const uint8_t*)d_dict, (const uint64_t*)(base + ZMI_SD_LAY_OFF), (const uint32_t*)(base + ZMI_SD_LAY_LEN), 1u, 1u,
                            (uint32_t*)(base + ZMI_SD_DICTID), nullptr, stream);
    }
    return 0;
}

// search / parse effort per level: the MI355X analogue of CONFIGURATION_TABLE
// (zlib-rs/src/deflate/algorithm/mod.rs:69-82).  Every position is searched in parallel, so the
// chain budget is what the slowest lane of a wave spends; see DESIGN.md for the measured trade-off.
struct zmi_level_cfg {
    uint32_t chain, nice, good, lazy, tok;
};
// chain = candidates examined per position (the 4-byte probe counts as one); tok = tokens per sub-block of the
// encoder's adaptive block splitting.  Round 2 moved the curve: 16-bit hash heads (twice the buckets: fewer candidates
// that are hash collisions), the probe as a slim 8-byte compare outside the chain loop, limits for short far matches
// that follow the data (encode.hip enc_far_limits), 128 KiB pieces.  Level 6 = budget 5: lcet10.txt 2.79 -> 2.85 (the
// reference's level 6: 2.91), benchmark shards 2.247 -> see DESIGN.md section 9.
static const zmi_level_cfg kLevels[10] = {
    {0, 0, 0, 0, 4096},          // 0: stored
    {2, 16, 8, 0, 8192},         // 1  (greedy, lazy path of the encoder)
    {3, 32, 8, 0, 8192},         // 2  (greedy)
    // 3 ... 9: the token choice is the cost parse's (csrc/parse.hip) -- `lazy` is not used there, what separates the levels is the
    // search: budget, and the length at which a walk is content (good)
    // (round 6: four distinct rungs, as the reference's table has -- deflate/algorithm/mod.rs:72-76.  CPU emulator, 512 KiB inputs, benchmark
    // mix / lcet10.txt: budget 2 = 2.2294 / 2.811, budget 3 good 8 = 2.2476 / 2.869, budget 3 good 16 = 2.2554 / 2.881, budget 4 = 2.2670 / 2.909;
    // until round 5 levels 4 and 5 were one configuration and level 3 ran level 4's search)
    {2, 32, 8, 4, 4096},         // 3
    {3, 64, 8, 8, 4096},         // 4  (a walk is content with 8 equal bytes)
    {3, 128, 16, 16, 4096},      // 5  (... with 16)
    {4, 128, 16, 32, 4096},      // 6  (good 32 -> 16 in round 4: lz77 138.7 -> 130.1 ms, ratio 2.2550 -> 2.2532, lcet10.txt -0.04 %)
    {6, 128, 16, 32, 4096},      // 7
    // 8, 9 (round 5): budgets 10 and 16 on the SHORT-budget kernel (the walk ends at the first candidate equal in 16 bytes, the wave
    // extends it afterwards) instead of 14 and 22 on the deep one, whose in-loop extension makes a candidate cost 22 ms against 7
    // (per 16 Ki shards).  Measured with the cost parse, 8192 shards (profiles/r05_level9_budget_sweep.txt): deep 22 = 2.325 at
    // 24.8 GiB/s, deep 12 = 2.319 at 35.4, short 16 = 2.319 at 39.5, short 10 = 2.314 at 49.2 (round 4's level 9, lazy parse, deep
    // 22: 2.315 at 26.0).  The deep instantiation is gone from lz77.hip.
    {10, 258, 16, 128, 2048},    // 8
    {16, 258, 16, 258, 2048},    // 9
};

extern "C" int zmi_checksum_batch_dev(zmi_ctx* c, const void* d_data, const uint64_t* d_off, const uint32_t* d_len,
                                      uint32_t n, int kind, uint32_t* d_adler, uint32_t* d_crc, void* stream) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (n == 0) return ZMI_E_OK;
    ZMI_ON_DEVICE(c);
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, (hipStream_t)stream);
        zmi_launch_checksum((const uint8_t*)d_data, d_off, d_len, n, (uint32_t)kind, d_adler, d_crc, (hipStream_t)stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_gen_shards_dev(zmi_ctx* c, void* d_out, uint64_t seed, uint32_t first_shard, uint32_t n_shards,
                                  uint32_t shard_bytes, void* stream) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (shard_bytes % 64u) return zmi_fail(ZMI_E_ARG, "shard_bytes must be a multiple of 64");
    ZMI_ON_DEVICE(c);
    zmi_launch_gen((uint8_t*)d_out, seed, first_shard, n_shards, shard_bytes, (hipStream_t)stream);
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_gen_shards_strided_dev(zmi_ctx* c, void* d_out, uint64_t seed, uint32_t first_shard, uint32_t shard_step,
                                          uint32_t n_shards, uint32_t shard_bytes, void* stream) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (shard_bytes % 64u) return zmi_fail(ZMI_E_ARG, "shard_bytes must be a multiple of 64");
    ZMI_ON_DEVICE(c);
    zmi_launch_gen_strided((uint8_t*)d_out, seed, first_shard, shard_step, n_shards, shard_bytes, (hipStream_t)stream);
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- the stitch: strided slots -> dense slab, slab -> globally ordered output (pack.hip) ----
extern "C" int zmi_scan_sizes_dev(zmi_ctx* c, const uint32_t* d_len, uint32_t n, uint64_t* d_off, void* stream) {
    if (!c || !d_off || (!d_len && n)) return zmi_fail(ZMI_E_ARG, "null argument");
    ZMI_ON_DEVICE(c);
    zmi_launch_scan_sizes(d_len, n, d_off, (hipStream_t)stream);
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}
extern "C" int zmi_copy_ranges_dev(zmi_ctx* c, const void* d_src, const uint64_t* d_src_off, uint64_t src_stride,
                                   const uint32_t* d_len, uint32_t n, uint32_t max_len, void* d_dst, const uint64_t* d_dst_off,
                                   uint64_t dst_cap, void* stream) {
    if (!c || !d_src || !d_len || !d_dst || !d_dst_off) return zmi_fail(ZMI_E_ARG, "null argument");
    if (n == 0) return ZMI_E_OK;
    ZMI_ON_DEVICE(c);
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, (hipStream_t)stream);
        zmi_launch_copy_ranges((const uint8_t*)d_src, d_src_off, src_stride, d_len, n, (uint8_t*)d_dst, d_dst_off, dst_cap, max_len,
                               (hipStream_t)stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}
extern "C" int zmi_pack_slab_dev(zmi_ctx* c, const void* d_slots, uint64_t slot_stride, const uint32_t* d_len, uint32_t n,
                                 void* d_slab, uint64_t slab_cap, uint64_t* d_off, void* stream) {
    int rc = zmi_scan_sizes_dev(c, d_len, n, d_off, stream);
    if (rc) return rc;
    const uint32_t max_len = slot_stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)slot_stride;
    return zmi_copy_ranges_dev(c, d_slots, nullptr, slot_stride, d_len, n, max_len, d_slab, d_off, slab_cap, stream);
}

// The encoder's worst case for one of `pieces` regions of a shard of max_len bytes: every block stored (5 header bytes + byte
// alignment); a block holds at least one sub-block of block_tokens tokens (>= as many input bytes), stored sub-blocks are cut at 32 KiB
static uint64_t zmi_enc_region_worst(uint64_t max_len, uint32_t pieces, uint32_t block_tokens, bool dictid) {
    const uint64_t psize = ((max_len + pieces - 1u) / pieces + 63u) & ~63ull;
    const uint64_t min_block = block_tokens < 32768u ? block_tokens : 32768u;
    return psize + 6u * (psize / min_block + 3u) + 32u + (dictid ? 4u : 0u);   // (the DICTID in the first piece)
}
// The regions a shard's slot is cut into (the encoder runs one wave per region: byte-aligned sub-streams, concatenated afterwards): one
// per block_span of max_len, at most 16, fewer where a region of out_stride / pieces could not hold its worst case
static uint32_t zmi_enc_regions(uint32_t max_len, uint64_t out_stride, uint32_t block_span, uint32_t block_tokens, bool dictid) {
    uint32_t pieces = (max_len + block_span - 1u) / block_span;
    if (pieces < 1u) pieces = 1u;
    if (pieces > 16u) pieces = 16u;
    const char* pieces_env = zmi_tune("ZMI_PIECES");
    if (pieces_env && atoi(pieces_env) >= 1 && atoi(pieces_env) <= 64) pieces = (uint32_t)atoi(pieces_env);
    // every piece region must hold its worst case (stored blocks + marker) and stay 16-byte aligned
    while (pieces > 1u && ((out_stride / pieces) & ~15ull) < zmi_enc_region_worst(max_len, pieces, block_tokens, dictid)) --pieces;
    return pieces;
}
// The slot of a piece of at most max_len bytes that is encoded in the regions of a piece_bytes shard (zmi_deflate_impl, geom_len =
// piece_bytes: bytes that depend on piece_bytes alone, slots that follow the data): zmi_deflate_pieces_stride(max_len), more only where
// sixteen regions' worst cases do not fit that (pieces of a few KiB)
static uint64_t zmi_piece_slot_stride(uint32_t max_len, uint32_t piece_bytes, int level) {
    const uint32_t regions = zmi_enc_regions(piece_bytes, zmi_deflate_pieces_stride(piece_bytes), 65536u, kLevels[level].tok, false);
    const uint64_t hold = (uint64_t)regions * ((zmi_enc_region_worst(max_len, regions, kLevels[level].tok, false) + 15u) & ~15ull);
    return std::max<uint64_t>(zmi_deflate_pieces_stride(max_len), hold);
}
// ZMI_STREAM_GROUP (tests, probes): the pieces per launch group, whatever the scratch limit says; 0: not set
static uint64_t zmi_group_override() {
    const char* gv = zmi_tune("ZMI_STREAM_GROUP");
    return gv && atoll(gv) > 0 ? (uint64_t)atoll(gv) : 0u;
}
// The launch groups of np pieces (zmi_scratch.h: one group's output slots and the encoder's match scratch together stay within the
// scratch limit) and one group's slots in c->sd_slots
static int zmi_plan_slots(zmi_ctx* c, uint64_t np, uint32_t max_len, uint64_t stride, const char* too_small, zmi_group_plan* plan) {
    *plan = zmi_plan_groups(c->scratch_limit, zmi_group_override(), np, max_len, stride);
    if (np && plan->group == 0) return zmi_fail(ZMI_E_NOMEM, too_small);
    return zmi_reserve(c->sd_slots, (size_t)(plan->group * stride));
}

// carry: -1 = what chain_mode implies, 0 = segments forget history (independent pieces of one stream), 1 = window carry-over.
// ends: chain mode 2 only, the device bitmap of the shards that end a stream (zmi_enc_params).  geom_len (0: max_len): the max_len whose
// region geometry the shards get -- that of a call with max_len = geom_len and the slots of zmi_deflate_pieces_stride(geom_len) --
// while scratch and slots are sized by the smaller max_len the shards really have (zmi_zip_write_dev: bytes that depend on piece_bytes
// alone, slots that follow the data); out_stride must then hold that geometry's regions for max_len.
// launch_n: the number of segments the small-launch rule below judges (0: n) -- the whole stream's when a stream is compressed in
// several launch groups, so that the bytes do not depend on the grouping.
struct zmi_def_req {   // (every call site names what it passes)
    const void* d_in = nullptr; const uint64_t* d_in_off = nullptr; const uint32_t* d_in_len = nullptr; uint32_t n = 0, max_len = 0;   // the shards
    int level = 0, strategy = 0, wrap = ZMI_WRAP_RAW; uint32_t chain_mode = 0, dict_len = 0, window_bits = 15;
    void* d_out = nullptr; uint64_t out_stride = 0; uint32_t* d_out_len = nullptr; int32_t* d_status = nullptr;                         // the slots
    void* stream = nullptr;
    int carry = -1; uint64_t launch_n = 0; const zmi_sd_deflate* sd = nullptr; const uint32_t* ends = nullptr; uint32_t geom_len = 0;   // (above)
};
static int zmi_deflate_impl(zmi_ctx* c, const zmi_def_req& q);

extern "C" int zmi_deflate_batch_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                     uint32_t n, uint32_t max_len, int level, int strategy, int wrap, void* d_out,
                                     uint64_t out_stride, uint32_t* d_out_len, int32_t* d_status, void* stream_) {
    return zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level,
                                .strategy = strategy, .wrap = wrap, .d_out = d_out, .out_stride = out_stride, .d_out_len = d_out_len,
                                .d_status = d_status, .stream = stream_});
}

// Every shard as deflateInit2_ + deflateSetDictionary(dict) + deflate(Z_FINISH) (zlib-rs/src/deflate.rs:499-564), one dictionary
// for the whole call; see include/zmi355.h.  chain_mode 0: a shard's bytes depend on the dictionary, its own bytes, level, strategy
// and wrap alone.
extern "C" int zmi_deflate_batch_shared_dict_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                 uint32_t n, uint32_t max_len, int level, int strategy, int wrap, const void* d_dict,
                                                 uint32_t dict_len, void* d_out, uint64_t out_stride, uint32_t* d_out_len,
                                                 int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap != ZMI_WRAP_RAW && wrap != ZMI_WRAP_ZLIB) return zmi_fail(ZMI_E_ARG, "a preset dictionary needs wrap raw or zlib (a gzip member has no dictionary field)");
    zmi_def_req q{.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level, .strategy = strategy,
                  .wrap = wrap, .d_out = d_out, .out_stride = out_stride, .d_out_len = d_out_len, .d_status = d_status, .stream = stream_};
    if (!d_dict || dict_len == 0u) return zmi_deflate_impl(c, q);
    if (level < -1 || level > 9) return zmi_fail(ZMI_E_ARG, "level must be -1..9");
    if (strategy < 0 || strategy > 4) return zmi_fail(ZMI_E_ARG, "strategy must be 0..4");
    if (out_stride % 16u || out_stride < zmi_deflate_dict_bound(max_len, wrap))
        return zmi_fail(ZMI_E_ARG, "out_stride must be a multiple of 16 and >= zmi_deflate_dict_bound(max_len)");
    if (n == 0) return ZMI_E_OK;
    zmi_sd_deflate sd;
    {
        ZMI_ON_DEVICE(c);
        const uint32_t img_len = zmi_lz77_dict_image_len(dict_len);
        int rc = zmi_sd_prepare(c, d_dict, dict_len, false, wrap == ZMI_WRAP_ZLIB, (hipStream_t)stream_, 0u, img_len, 16u);
        if (rc) return rc;
        sd.img = (const uint8_t*)c->dict.p + ZMI_SD_DEF_IMG;
        sd.img_len = img_len;
        sd.dictid = (const uint32_t*)((const uint8_t*)c->dict.p + ZMI_SD_DICTID);
    }
    q.sd = &sd;
    return zmi_deflate_impl(c, q);
}

// The shards are consecutive segments of ONE raw deflate stream, contiguous in d_in (d_in_off[i+1] = d_in_off[i] +
// d_in_len[i]).  Every segment starts byte aligned (the empty stored block of Z_SYNC_FLUSH,
// zlib-rs/src/deflate.rs:2733-2738) and may match into the up to 27 KiB in front of it (window carry-over), so
// splitting a stream costs no cold start; `finish` != 0 makes the last shard end the stream (BFINAL).
extern "C" int zmi_deflate_chain_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                     uint32_t n, uint32_t max_len, int level, int strategy, int finish, void* d_out,
                                     uint64_t out_stride, uint32_t* d_out_len, int32_t* d_status, void* stream_) {
    return zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level,
                                .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = finish ? 1u : 2u, .d_out = d_out,
                                .out_stride = out_stride, .d_out_len = d_out_len, .d_status = d_status, .stream = stream_});
}

// As zmi_deflate_chain_dev; additionally the dict_len bytes in front of the first segment (d_in + d_in_off[0] -
// dict_len ...) are history the stream may match into: a preset dictionary (deflateSetDictionary,
// zlib-rs/src/deflate.rs:499-564) or the tail of the input compressed by an earlier call on the same stream.
extern "C" int zmi_deflate_chain_dict_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                          uint32_t n, uint32_t max_len, int level, int strategy, int finish, uint32_t dict_len,
                                          void* d_out, uint64_t out_stride, uint32_t* d_out_len, int32_t* d_status,
                                          void* stream_) {
    return zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level,
                                .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = finish ? 1u : 2u, .dict_len = dict_len, .d_out = d_out,
                                .out_stride = out_stride, .d_out_len = d_out_len, .d_status = d_status, .stream = stream_});
}

// The chained form for a stream opened with windowBits < 15 (deflateInit2_, zlib-rs/src/deflate.rs:252-312): no
// back-reference may reach farther than the reference's max_dist = 2^windowBits - MIN_LOOKAHEAD (deflate.rs:1423-1425),
// or an inflater that allocates the window the header announces rejects the stream ("invalid distance too far back").
extern "C" int zmi_deflate_chain_window_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                            uint32_t n, uint32_t max_len, int level, int strategy, int finish, uint32_t dict_len,
                                            uint32_t window_bits, void* d_out, uint64_t out_stride, uint32_t* d_out_len,
                                            int32_t* d_status, void* stream_) {
    if (window_bits < 9u || window_bits > 15u) return zmi_fail(ZMI_E_ARG, "window_bits must be 9..15");
    return zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level,
                                .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = finish ? 1u : 2u, .dict_len = dict_len, .window_bits = window_bits,
                                .d_out = d_out, .out_stride = out_stride, .d_out_len = d_out_len, .d_status = d_status, .stream = stream_});
}

static int zmi_deflate_impl(zmi_ctx* c, const zmi_def_req& q) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    const int level = q.level == -1 ? 6 : q.level;
    const uint32_t n = q.n;
    const zmi_sd_deflate* const sd = q.sd;
    if (level < 0 || level > 9) return zmi_fail(ZMI_E_ARG, "level must be -1..9");
    if (q.strategy < 0 || q.strategy > 4) return zmi_fail(ZMI_E_ARG, "strategy must be 0..4");
    if (q.wrap < ZMI_WRAP_RAW || q.wrap > ZMI_WRAP_GZIP) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip");
    if (q.out_stride % 16u || q.out_stride < (sd ? zmi_deflate_dict_bound(q.max_len, q.wrap) : zmi_deflate_bound(q.max_len, q.wrap)))
        return zmi_fail(ZMI_E_ARG, sd ? "out_stride must be a multiple of 16 and >= zmi_deflate_dict_bound(max_len)"
                                      : "out_stride must be a multiple of 16 and >= zmi_deflate_bound(max_len)");
    if (q.out_stride > 0xFFFFFFF0ull) return zmi_fail(ZMI_E_ARG, "shards larger than 3.5 GiB are not supported");
    if (n == 0) return ZMI_E_OK;
    hipStream_t stream = (hipStream_t)q.stream;
    ZMI_ON_DEVICE(c);

    // wrapper checksums
    int rc = zmi_reserve(c->sums, (size_t)n * 8u);
    if (rc) return rc;
    uint32_t* d_adler = (uint32_t*)c->sums.p;
    uint32_t* d_crc = d_adler + n;
    uint32_t kind = q.wrap == ZMI_WRAP_ZLIB ? 1u : (q.wrap == ZMI_WRAP_GZIP ? 2u : 0u);
    // The checksums are needed by the encoder's trailers only: they run on a side stream beside the match search (one is
    // HBM-bound, the other instruction-bound; in a launch of a few hundred shards the checksum kernel is one workgroup per
    // shard with nothing to hide its latency behind: 4.5 ms in front of 6.4 ms of lz77 for 512 shards) and join in front of
    // the first encode launch.
    bool forked = false;
    struct join_guard { zmi_ctx* c; hipStream_t st; bool& f; ~join_guard() { if (f) (void)hipStreamWaitEvent(st, c->ev_join, 0); } } join_on_exit{c, stream, forked};
    if (kind) {
        if (!c->side) {
            ZMI_HIP(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
            ZMI_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
            ZMI_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
        }
        ZMI_HIP(hipEventRecord(c->ev_fork, stream));
        ZMI_HIP(hipStreamWaitEvent(c->side, c->ev_fork, 0));
        {
            zmi_scope_timer tm(c, ZMI_K_CHECKSUM, c->side);
            zmi_launch_checksum((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, n, kind, d_adler, d_crc, c->side);
        }
        ZMI_HIP(hipEventRecord(c->ev_join, c->side));
        forked = true;
    }

    const zmi_level_cfg& L = kLevels[level];
    zmi_lz_params lp;
    lp.max_chain = L.chain;
    lp.nice_len = L.nice;
    lp.good_len = L.good;
    lp.max_dist = 32768u;  // clamped to the ring-buffer limit by the launcher
    if (q.window_bits < 15u) lp.max_dist = (1u << q.window_bits) - 262u;   // w_size - MIN_LOOKAHEAD (deflate.rs:1423-1425)
    lp.hash6 = 1u;  // 6-byte-hash chain + one 4-byte probe: ~1.5x fewer chain steps than a 4-byte chain at equal ratio
    lp.claim = 64u;
    const char* claim_env = zmi_tune("ZMI_CLAIM");
    if (claim_env) lp.claim = (uint32_t)atoi(claim_env);
    const char* md_env = zmi_tune("ZMI_MAXDIST");
    if (md_env && atoi(md_env) > 0 && (uint32_t)atoi(md_env) < lp.max_dist) lp.max_dist = (uint32_t)atoi(md_env);
    const char* h6_env = zmi_tune("ZMI_HASH6");
    if (h6_env) lp.hash6 = atoi(h6_env) ? 1u : 0u;
    zmi_enc_params ep;
    ep.max_lazy = L.lazy;
    ep.lazy2 = 1u;
    ep.lazy3 = 2u;
    if (const char* l3 = zmi_tune("ZMI_LAZY3")) ep.lazy3 = (uint32_t)atoi(l3);
    if (const char* l2 = zmi_tune("ZMI_LAZY2")) ep.lazy2 = (uint32_t)atoi(l2);
    ep.wrap = (uint32_t)q.wrap;
    ep.level = (uint32_t)level;
    ep.block_span = 65536u;    // one encoder wave per 64 KiB piece, 16 per 1 MiB shard (128 KiB pieces: +0.15 % ratio, but 137 -> 161 ms
                               // per 16 Ki shards: fewer, longer waves fill the chip worse)
    ep.strategy = (uint32_t)q.strategy;
    ep.chain_mode = q.chain_mode;
    ep.last_shard = n - 1u;
    ep.ends = q.chain_mode == 2u ? q.ends : nullptr;
    ep.dictid = (sd && q.wrap == ZMI_WRAP_ZLIB) ? sd->dictid : nullptr;
    if (level == 0) ep.strategy = 100u;           // stored blocks only (deflate_stored)
    ep.cost_parse = (level >= 3 && q.strategy != 2) ? 1u : 0u;
    if (const char* cp = zmi_tune("ZMI_COST_PARSE")) ep.cost_parse = atoi(cp) ? 1u : 0u;
    if (q.strategy == 2) { lp.max_chain = 0; lp.max_dist = 0; } // Z_HUFFMAN_ONLY: literals only -- with no distance allowed no
                                                                 // position gets a candidate (a zero chain budget alone still
                                                                 // examines the first one)
    if (q.strategy == 3) lp.max_dist = 1;         // Z_RLE: distance-1 matches only
    const char* chain_env = zmi_tune("ZMI_CHAIN");  // tuning aid: override the chain budget of the selected level
    if (chain_env && atoi(chain_env) > 0 && level > 0 && q.strategy != 2) lp.max_chain = (uint32_t)atoi(chain_env);
    const char* good_env = zmi_tune("ZMI_GOOD");
    if (good_env && atoi(good_env) > 0) lp.good_len = (uint32_t)atoi(good_env);
    const char* nice_env = zmi_tune("ZMI_NICE");
    if (nice_env && atoi(nice_env) > 0) lp.nice_len = (uint32_t)atoi(nice_env);
    const char* lazy_env = zmi_tune("ZMI_LAZY");
    if (lazy_env && atoi(lazy_env) >= 0) ep.max_lazy = (uint32_t)atoi(lazy_env);
    lp.carry = q.chain_mode != 0u ? 1u : 0u;   // segments of one stream: a segment sees the window in front of it
    lp.dict_len = q.chain_mode != 0u ? q.dict_len : 0u;
    if (const char* cv = zmi_tune("ZMI_CARRY")) lp.carry = (q.chain_mode != 0u && atoi(cv)) ? 1u : 0u;
    if (q.carry >= 0) lp.carry = (q.chain_mode != 0u && q.carry) ? 1u : 0u;
    // hash-building waves: 1 for the deep chains (the searchers are the whole kernel there), 2 for the short ones (14 searcher
    // waves outrun one producer: budget 5 measured 227 ms with two, 273 ms with one), 3 at level 1, whose searchers do so
    // little per position that even two producers set the pace (97.1 -> 95.2 ms per 16 Ki shards; at level 3 a third
    // producer already costs more as a missing searcher than it brings: 114.2 -> 120.5 ms)
    lp.producers = L.chain > 8u ? 1u : (L.chain <= 2u ? 3u : 2u);   // (budgets 10 / 16: one producer measured 1-2 % ahead of two)
    if (const char* pv = zmi_tune("ZMI_PRODUCERS")) lp.producers = (uint32_t)atoi(pv);
    lp.dbg = 0u;
    if (const char* dv = zmi_tune("ZMI_LZ_DBG")) lp.dbg = (uint32_t)atoi(dv);
    lp.barren_chain = 1u;
    if (const char* bv = zmi_tune("ZMI_BARREN_CHAIN")) lp.barren_chain = (uint32_t)atoi(bv);
    // short far matches are judged by the encoder, block by block, from the codes it just used (enc_far_limits); the
    // search reports every match of 4+ bytes
    lp.far4 = 32768u;
    lp.far5 = 32768u;
    ep.far4 = 2048u;    // the first block of a piece, before any code exists
    ep.far5 = 16384u;
    if (const char* f4 = zmi_tune("ZMI_FAR4")) ep.far4 = (uint32_t)atoi(f4);
    if (const char* f5 = zmi_tune("ZMI_FAR5")) ep.far5 = (uint32_t)atoi(f5);
    ep.block_tokens = L.tok;
    ep.split_hdr_bits = 640u;
    ep.min_sub_span = L.tok >= 4096u ? 5120u : 0u;   // (levels 8 and 9 cut finer, 2048 tokens, and keep every block they can get)
                               // literal-dense data: a sub-block of 4096 tokens is little more than 4 KiB of input, and a block of its own
                               // is a full tree construction; measured on the benchmark mix: 0 -> 103.3 ms encode at ratio 2.2635, 5120 ->
                               // 98.9 ms at 2.2567, 8192 -> 94.6 ms at 2.2440
    if (const char* ms = zmi_tune("ZMI_MIN_SUB_SPAN")) ep.min_sub_span = (uint32_t)atoi(ms);
    if (const char* hb = zmi_tune("ZMI_SPLIT_HDR")) ep.split_hdr_bits = (uint32_t)atoi(hb);
    if (const char* bt = zmi_tune("ZMI_BLOCK_TOKENS")) ep.block_tokens = (uint32_t)atoi(bt) >= 64u ? (uint32_t)atoi(bt) : 64u;
    // a launch of a few shards -- the 64 KiB segments of one deflate() call, a compress2() -- would be a few dozen encoder waves of
    // 0.7 ... 1.8 ms each on 256 CUs (profiles/r05_stream_deflate_trace.txt): pieces of 8 KiB there, eight waves per segment
    // (a marker and a fresh block per 8 KiB, only where the chip would otherwise stand empty: the 15 MiB stream of
    // tools/gpu_stream_deflate_probe.py 2.3362 with 16 KiB pieces -- 0.2 ... 0.5 ms of encoder per 4 MiB call --, 2.3304 with 8 KiB,
    // 2.3076 with 4 KiB)
    // (only for the segments of ONE stream -- chain mode: what a batch of independent shards compresses to does not depend on how
    // many of them a launch holds, tests/test_gpu_parity.py::test_host_batch_pipeline_on_gpu)
    // (independent pieces of a single stream, carry 0, never: a piece's bytes depend on its own input alone, whichever GPU and
    // whichever launch compresses it -- zmi_deflate_stream_dev)
    const bool small_launch = q.chain_mode != 0u && q.carry != 0 && (q.launch_n ? q.launch_n : n) * ((q.max_len + 65535u) / 65536u) < 512u;
    if (small_launch) ep.block_span = 8192u;
    const char* span_env = zmi_tune("ZMI_BLOCK_SPAN");
    if (span_env && atoi(span_env) >= 64) ep.block_span = (uint32_t)atoi(span_env);

    // match/token scratch: one u32 per position, shards padded to a multiple of 64 positions; with the cost parse two more bits
    // per position behind it (its decisions, 16 bytes per 64 positions)
    const uint64_t stride = ((uint64_t)q.max_len + 63u) & ~63ull;
    uint64_t per_shard = (stride ? stride : 64u) * 4u;
    const uint64_t dec_bytes = ep.cost_parse ? per_shard / 16u : 0u;
    uint64_t group = c->scratch_limit / (per_shard + dec_bytes);
    if (group == 0) return zmi_fail(ZMI_E_NOMEM, "scratch limit too small for one shard");
    if (group > n) group = n;
    rc = zmi_reserve(c->match, (size_t)(group * (per_shard + dec_bytes)));
    if (rc) return rc;
    uint32_t* const d_dec = ep.cost_parse ? (uint32_t*)((uint8_t*)c->match.p + group * per_shard) : nullptr;
    uint32_t pieces = zmi_enc_regions(q.max_len, q.out_stride, ep.block_span, ep.block_tokens, sd != nullptr);
    if (q.geom_len) {
        pieces = zmi_enc_regions(q.geom_len, zmi_deflate_pieces_stride(q.geom_len), ep.block_span, ep.block_tokens, sd != nullptr);
        if (((q.out_stride / pieces) & ~15ull) < zmi_enc_region_worst(q.max_len, pieces, ep.block_tokens, sd != nullptr))
            return zmi_fail(ZMI_E_ARG, "out_stride does not hold the regions of geom_len");
    }
    rc = zmi_reserve(c->pieces, (size_t)n * pieces * 4u);
    if (rc) return rc;
    for (uint64_t first = 0; first < n; first += group) {
        uint32_t cnt = (uint32_t)((n - first < group) ? (n - first) : group);
        {
            zmi_scope_timer tm(c, ZMI_K_LZ77, stream);
            int lrc = (sd && sd->img_len)
                          ? zmi_launch_lz77_dict((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, (uint32_t)first, cnt, (uint32_t*)c->match.p,
                                                 per_shard / 4u, lp, sd->img, sd->img_len, stream)
                          : zmi_launch_lz77((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, (uint32_t)first, cnt, (uint32_t*)c->match.p,
                                            per_shard / 4u, lp, stream);
            if (lrc) return zmi_fail(ZMI_E_HIP, "lz77 launch setup", (hipError_t)lrc);
        }
        if (ep.cost_parse) {
            zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
            zmi_launch_parse(q.d_in_len, (uint32_t)first, cnt, q.max_len, (const uint32_t*)c->match.p, per_shard / 4u, d_dec, dec_bytes / 4u, pieces,
                             (uint32_t)q.strategy, small_launch ? 4u : 64u, stream);
        }
        if (forked) { ZMI_HIP(hipStreamWaitEvent(stream, c->ev_join, 0)); forked = false; }
        zmi_scope_timer tm2(c, ZMI_K_ENCODE, stream);
        zmi_launch_encode((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, (uint32_t)first, cnt, (uint32_t*)c->match.p,
                          per_shard / 4u, d_adler, d_crc, (uint8_t*)q.d_out, q.out_stride, (uint32_t)q.out_stride, q.d_out_len,
                          q.d_status, pieces, (uint32_t*)c->pieces.p, d_dec, dec_bytes / 4u, ep, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- single-stream deflate (pigz-style): one raw / zlib / gzip stream from many pieces -----------------------------------------
// The reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221 (split_deflate): every piece but the last ends with
// the empty stored block of a flush (Z_SYNC_FLUSH, deflate.rs:2733-2738; Z_FULL_FLUSH also forgets history, :2739-2752), the
// wrapper appears once, and the trailer carries the combined check value (crc32/combine.rs:3-13, adler32.rs:58).  Here the pieces
// are the segments of the chained encoder, the checks are combined by a reduction on the device (checksum.hip) and the frame is
// written by a kernel (pack.hip): no host round trip anywhere.
extern "C" uint64_t zmi_deflate_pieces_stride(uint32_t max_len) { return zmi_deflate_bound(max_len, ZMI_WRAP_RAW) + 16u; }
extern "C" uint32_t zmi_stream_header_bytes(int wrap) { return zmi_stream_header_len(wrap); }

extern "C" uint64_t zmi_deflate_stream_bound(uint64_t n, uint32_t piece_bytes, int wrap) {
    if (piece_bytes == 0) return 0;
    const uint64_t np = n ? (n + piece_bytes - 1u) / piece_bytes : 1u;
    const uint32_t max_len = n < piece_bytes ? (uint32_t)n : piece_bytes;
    return np * zmi_deflate_pieces_stride(max_len) + zmi_stream_header_len(wrap) + (wrap == ZMI_WRAP_ZLIB ? 4u : (wrap == ZMI_WRAP_GZIP ? 8u : 0u));
}

// d_check[i] = Adler-32 (zlib) / CRC-32 (gzip) of piece i's raw bytes; nothing for raw
static int zmi_piece_checks(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, int wrap,
                            uint32_t* d_check, hipStream_t stream) {
    if (wrap == ZMI_WRAP_RAW || n == 0) return ZMI_E_OK;
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_checksum((const uint8_t*)d_in, d_in_off, d_in_len, n, wrap == ZMI_WRAP_ZLIB ? 1u : 2u, d_check, d_check, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_deflate_pieces_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                      uint32_t max_len, int level, int strategy, int wrap, uint32_t flags, int final_piece,
                                      void* d_out, uint64_t out_stride, uint32_t* d_out_len, uint32_t* d_check, int32_t* d_status,
                                      void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (flags & ~(uint32_t)ZMI_STREAM_INDEPENDENT) return zmi_fail(ZMI_E_ARG, "zmi_deflate_pieces_dev: unknown flags");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_GZIP) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip");
    if (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_len || !d_status || (wrap != ZMI_WRAP_RAW && !d_check)))
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (out_stride < zmi_deflate_pieces_stride(max_len)) return zmi_fail(ZMI_E_ARG, "out_stride must be >= zmi_deflate_pieces_stride(max_len)");
    if (n == 0) return ZMI_E_OK;
    const bool indep = (flags & ZMI_STREAM_INDEPENDENT) != 0u;
    ZMI_ON_DEVICE(c);
    hipStream_t stream = (hipStream_t)stream_;
    int rc = zmi_piece_checks(c, d_in, d_in_off, d_in_len, n, wrap, d_check, stream);
    if (rc) return rc;
    return zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .max_len = max_len, .level = level,
                                .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = final_piece ? 1u : 2u, .d_out = d_out, .out_stride = out_stride,
                                .d_out_len = d_out_len, .d_status = d_status, .stream = stream_, .carry = indep ? 0 : 1});
}

extern "C" int zmi_checksum_combine_dev(zmi_ctx* c, int wrap, const uint32_t* d_check, const uint32_t* d_len, uint32_t world,
                                        uint32_t n_local, uint32_t* d_out_check, uint64_t* d_out_len, void* stream) {
    if (!c || (!d_out_check && !d_out_len)) return zmi_fail(ZMI_E_ARG, "null argument");
    if (wrap != ZMI_WRAP_ZLIB && wrap != ZMI_WRAP_GZIP) return zmi_fail(ZMI_E_ARG, "zmi_checksum_combine_dev: wrap must be zlib or gzip");
    const uint64_t n64 = (uint64_t)world * n_local;
    if (world == 0 || n64 > 0xFFFFFFFFull) return zmi_fail(ZMI_E_ARG, "zmi_checksum_combine_dev: world * n_local must be 1 .. 2^32 - 1 entries");
    if (n64 && (!d_check || !d_len)) return zmi_fail(ZMI_E_ARG, "null argument");
    ZMI_ON_DEVICE(c);
    const uint32_t n = (uint32_t)n64, nb = zmi_combine_partials(n);
    // partials: nb u64 lengths | a u64 | nb u32 checks | a u32 (the u64 / u32 stand in for a result the caller does not want)
    int rc = zmi_reserve(c->comb, (size_t)nb * 12u + 12u);
    if (rc) return rc;
    uint64_t* pl = (uint64_t*)c->comb.p;
    uint32_t* pc = (uint32_t*)(pl + nb + 1u);
    uint64_t* rl = d_out_len ? d_out_len : pl + nb;
    uint32_t* rc_ = d_out_check ? d_out_check : pc + nb;
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, (hipStream_t)stream);
        zmi_launch_checksum_combine(d_check, d_len, n, world, n_local, wrap == ZMI_WRAP_ZLIB ? 1u : 0u, pc, pl, rc_, rl, (hipStream_t)stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_stream_frame_dev(zmi_ctx* c, int wrap, int level, int strategy, const uint64_t* d_payload_len, const uint32_t* d_check,
                                    const uint64_t* d_raw_len, void* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_status,
                                    void* stream) {
    if (!c || !d_payload_len || !d_out || !d_out_len) return zmi_fail(ZMI_E_ARG, "null argument");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_GZIP) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip");
    if (wrap != ZMI_WRAP_RAW && !d_check) return zmi_fail(ZMI_E_ARG, "zmi_stream_frame_dev: the check value is needed");
    if (wrap == ZMI_WRAP_GZIP && !d_raw_len) return zmi_fail(ZMI_E_ARG, "zmi_stream_frame_dev: gzip needs the raw length (ISIZE)");
    if (level == -1) level = 6;
    if (level < 0 || level > 9 || strategy < 0 || strategy > 4) return zmi_fail(ZMI_E_ARG, "level must be -1..9, strategy 0..4");
    ZMI_ON_DEVICE(c);
    if (d_status) ZMI_HIP(hipMemsetAsync(d_status, 0, 4, (hipStream_t)stream));
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, (hipStream_t)stream);
        zmi_launch_frame((uint8_t*)d_out, out_cap, (uint32_t)wrap, (uint32_t)level, (uint32_t)strategy, d_payload_len, d_check, d_raw_len,
                         d_out_len, d_status, nullptr, 0u, nullptr, 0u, (hipStream_t)stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_deflate_stream_dev(zmi_ctx* c, const void* d_in, uint64_t n, uint32_t piece_bytes, int level, int strategy, int wrap,
                                      uint32_t flags, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_piece_off,
                                      int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    int rc = zmi_check_piece_bytes(piece_bytes);
    if (rc) return rc;
    if (flags & ~(uint32_t)ZMI_STREAM_INDEPENDENT) return zmi_fail(ZMI_E_ARG, "zmi_deflate_stream_dev: unknown flags");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_GZIP) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip");
    rc = zmi_check_level_strategy(level, strategy);
    if (rc) return rc;
    if ((n && !d_in) || !d_out || !d_out_len || !d_status) return zmi_fail(ZMI_E_ARG, "null argument");
    const uint64_t np64 = n ? (n + piece_bytes - 1u) / piece_bytes : 1u;
    if (np64 > 0x7FFFFFFFull) return zmi_fail(ZMI_E_ARG, "zmi_deflate_stream_dev: more than 2^31 - 1 pieces");
    const uint32_t np = (uint32_t)np64;
    const bool indep = (flags & ZMI_STREAM_INDEPENDENT) != 0u;
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);

    uint64_t *d_off, *d_poff, *d_raw;
    uint32_t *d_len, *d_olen, *d_chk, *d_comb;
    int32_t* d_st;
    rc = zmi_carve(c->sd_meta, [&](zmi_carver k) {
        k.take(np, d_off);                                  // the pieces' places in d_in
        k.take_unless(d_piece_off, np + 1u, d_poff);        // ... in the payload (the caller's index holds them if there is one)
        k.take(1u, d_raw);                                  // the raw total
        k.take(np, d_len, d_olen, d_st, d_chk);             // per piece: raw and compressed size, status, check value
        k.take(1u, d_comb);                                 // the combined check
        k.skip(12u);                                        // (spare: the reservation has always ended with it)
        return k.end();
    });
    if (rc) return rc;

    const uint32_t max_len = n < piece_bytes ? (uint32_t)n : piece_bytes;
    const uint64_t stride = zmi_deflate_pieces_stride(max_len);
    zmi_group_plan plan;
    rc = zmi_plan_slots(c, np, max_len, stride, "scratch limit too small for one piece", &plan);
    if (rc) return rc;
    const uint64_t group = plan.group;

    ZMI_HIP(hipMemsetAsync(d_status, 0, 4, stream));
    ZMI_HIP(hipMemsetAsync(d_poff, 0, 8, stream));   // where the first group's pack starts
    zmi_launch_piece_layout(n, piece_bytes, np, d_off, d_len, stream);
    rc = zmi_piece_checks(c, d_in, d_off, d_len, np, wrap, d_chk, stream);
    if (rc) return rc;
    const uint32_t h = zmi_stream_header_len(wrap);
    uint8_t* const payload = (uint8_t*)d_out + h;
    const uint64_t payload_cap = out_cap > h ? out_cap - h : 0u;
    for (uint64_t first = 0; first < np; first += group) {
        const uint32_t cnt = (uint32_t)(np - first < group ? np - first : group);
        const bool last = first + cnt == np;
        // carry-over across a group boundary: the group's first piece sees the history in front of it (lz77.hip reads it as
        // dict_len bytes in front of the launch's first segment; anything beyond the window is the same as a full window)
        const uint64_t before = indep ? 0u : first * (uint64_t)piece_bytes;
        rc = zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_off + first, .d_in_len = d_len + first, .n = cnt, .max_len = max_len, .level = level,
                                  .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = last ? 1u : 2u,
                                  .dict_len = (uint32_t)(before < 65536u ? before : 65536u), .d_out = c->sd_slots.p, .out_stride = stride,
                                  .d_out_len = d_olen + first, .d_status = d_st + first, .stream = stream_, .carry = indep ? 0 : 1, .launch_n = np});
        if (rc) return rc;
        // the group's pieces go behind the previous group's, the running offset never leaves the device
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_scan_sizes_base(d_olen + first, cnt, d_poff + first, d_poff + first, stream);
        zmi_launch_copy_ranges((const uint8_t*)c->sd_slots.p, nullptr, stride, d_olen + first, cnt, payload, d_poff + first, payload_cap,
                               stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride, stream);
    }
    if (wrap != ZMI_WRAP_RAW) {
        rc = zmi_checksum_combine_dev(c, wrap, d_chk, d_len, 1u, np, d_comb, d_raw, stream_);
        if (rc) return rc;
    }
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_frame((uint8_t*)d_out, out_cap, (uint32_t)wrap, (uint32_t)level, (uint32_t)strategy, d_poff + np, d_comb, d_raw, d_out_len,
                         d_status, d_st, np, d_piece_off, d_piece_off ? np + 1u : 0u, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- BGZF: blocked gzip with a block index (include/zmi355.h; the kernels: pack.hip) ---------------------------------------------
// Every block is one shard of the batch encoder (chain mode 0, raw, one piece: max_len <= 65280 < block_span), framed by the pack
// kernel with htslib's header; the launch groups, the device-resident running offset and the ZMI_STREAM_GROUP knob are
// zmi_deflate_stream_dev's.
extern "C" uint64_t zmi_bgzf_bound(uint64_t n, uint32_t block_bytes) {
    if (block_bytes == 0) return 0;
    const uint64_t nb = n / block_bytes + (n % block_bytes ? 1u : 0u);
    return n + nb * (ZMI_BGZF_HEADER + 5u + 8u) + ZMI_BGZF_EOF;
}

// Blocks d_len[0 .. n) (every length <= max_len <= ZMI_BGZF_BLOCK_MAX: the callers saw to that) framed and packed into d_out from
// *d_boff on, which the caller zeroed; d_boff[1 .. n] and d_blen[0 .. n) are written.  The body's own tables are part of the caller's
// layout (zmi_bgzf_tabs).  The first non-zero encoder status lands in *d_status.
struct zmi_bgzf_tabs {
    uint32_t *olen, *crc, *stored;
    int32_t* st;
    // the encoder's sizes and statuses, the blocks' CRC-32 values, the stored flags
    void take(zmi_carver& k, size_t n) { k.take(n, olen, st, crc, stored); }
};
static int zmi_bgzf_body(zmi_ctx* c, const void* d_in, const uint64_t* d_off, const uint32_t* d_len, uint32_t n, uint32_t max_len, int level,
                         int strategy, void* d_out, uint64_t out_cap, uint64_t* d_boff, uint32_t* d_blen, const zmi_bgzf_tabs& tab, int32_t* d_status,
                         hipStream_t stream) {
    if (n == 0) return ZMI_E_OK;
    uint32_t *const d_olen = tab.olen, *const d_crc = tab.crc, *const d_stored = tab.stored;
    int32_t* const d_st = tab.st;
    // (a block's slot is the batch encoder's bound, not the slot of a stream's piece)
    const uint64_t stride = zmi_deflate_bound(max_len, ZMI_WRAP_RAW);
    zmi_group_plan plan;
    int rc = zmi_plan_slots(c, n, max_len, stride, "scratch limit too small for one block", &plan);
    if (rc) return rc;
    const uint64_t group = plan.group;
    rc = zmi_piece_checks(c, d_in, d_off, d_len, n, ZMI_WRAP_GZIP, d_crc, stream);
    if (rc) return rc;
    for (uint64_t first = 0; first < n; first += group) {
        const uint32_t cnt = (uint32_t)(n - first < group ? n - first : group);
        rc = zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_off + first, .d_in_len = d_len + first, .n = cnt, .max_len = max_len, .level = level,
                                  .strategy = strategy, .wrap = ZMI_WRAP_RAW, .d_out = c->sd_slots.p, .out_stride = stride,
                                  .d_out_len = d_olen + first, .d_status = d_st + first, .stream = stream});
        if (rc) return rc;
        // the group's blocks go behind the previous group's, the running offset never leaves the device
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_bgzf_sizes(d_len + first, d_olen + first, d_st + first, cnt, d_blen + first, d_stored + first, d_status, stream);
        zmi_launch_scan_sizes_base(d_blen + first, cnt, d_boff + first, d_boff + first, stream);
        zmi_launch_bgzf_pack((const uint8_t*)d_in, d_off + first, d_len + first, (const uint8_t*)c->sd_slots.p, stride, d_olen + first,
                             d_stored + first, d_crc + first, cnt, max_len, (uint8_t*)d_out, d_boff + first, out_cap, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_bgzf_blocks_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                   uint32_t max_len, int level, int strategy, void* d_out, uint64_t out_cap, uint64_t* d_block_off,
                                   uint32_t* d_block_len, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (max_len > ZMI_BGZF_BLOCK_MAX) return zmi_fail(ZMI_E_ARG, "zmi_bgzf_blocks_dev: max_len must be <= ZMI_BGZF_BLOCK_MAX");
    int rc = zmi_check_level_strategy(level, strategy);
    if (rc) return rc;
    if (!d_block_off || !d_status || (out_cap && !d_out) || (n && (!d_in_off || !d_in_len || (max_len && !d_in))))
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (n > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "zmi_bgzf_blocks_dev: more than 2^31 - 1 blocks");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    uint32_t *d_len, *d_blen;
    zmi_bgzf_tabs tab;
    rc = zmi_carve(c->sd_meta, [&](zmi_carver k) {
        k.take(n, d_len);                            // the checked lengths
        k.take_unless(d_block_len, n, d_blen);       // the block sizes (the caller's table holds them if there is one)
        tab.take(k, n);
        k.skip(16u);                                 // (spare: the reservation has always ended with it)
        return k.end();
    });
    if (rc) return rc;
    ZMI_HIP(hipMemsetAsync(d_status, 0, 4, stream));
    ZMI_HIP(hipMemsetAsync(d_block_off, 0, 8, stream));
    zmi_launch_bgzf_lens(d_in_len, n, max_len, d_len, d_status, stream);
    rc = zmi_bgzf_body(c, d_in, d_in_off, d_len, n, max_len, level, strategy, d_out, out_cap, d_block_off, d_blen, tab, d_status, stream);
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_bgzf_close((uint8_t*)d_out, out_cap, d_block_off + n, 0u, nullptr, d_status, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_bgzf_deflate_dev(zmi_ctx* c, const void* d_in, uint64_t n, uint32_t block_bytes, int level, int strategy, void* d_out,
                                    uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_block_off, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (block_bytes == 0 || block_bytes > ZMI_BGZF_BLOCK_MAX) return zmi_fail(ZMI_E_ARG, "zmi_bgzf_deflate_dev: block_bytes must be 1 .. ZMI_BGZF_BLOCK_MAX");
    int rc = zmi_check_level_strategy(level, strategy);
    if (rc) return rc;
    if ((n && !d_in) || (out_cap && !d_out) || !d_out_len || !d_status) return zmi_fail(ZMI_E_ARG, "null argument");
    const uint64_t nb64 = n / block_bytes + (n % block_bytes ? 1u : 0u);
    if (nb64 > 0x7FFFFFFFull) return zmi_fail(ZMI_E_ARG, "zmi_bgzf_deflate_dev: more than 2^31 - 1 blocks");
    const uint32_t nb = (uint32_t)nb64;
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    uint64_t *d_off, *d_boff;
    uint32_t *d_len, *d_blen;
    zmi_bgzf_tabs tab;
    rc = zmi_carve(c->sd_meta, [&](zmi_carver k) {
        k.take(nb, d_off);                           // the blocks' places in d_in
        k.take_unless(d_block_off, nb + 1u, d_boff); // ... in the file (the caller's index holds them if there is one)
        k.take(nb, d_len);
        k.take(nb, d_blen);                          // the block sizes
        tab.take(k, nb);
        k.skip(16u);                                 // (spare: the reservation has always ended with it)
        return k.end();
    });
    if (rc) return rc;
    ZMI_HIP(hipMemsetAsync(d_status, 0, 4, stream));
    ZMI_HIP(hipMemsetAsync(d_boff, 0, 8, stream));   // where the first group's pack starts
    zmi_launch_piece_layout(n, block_bytes, nb, d_off, d_len, stream);
    const uint32_t max_len = n < block_bytes ? (uint32_t)n : block_bytes;
    rc = zmi_bgzf_body(c, d_in, d_off, d_len, nb, max_len, level, strategy, d_out, out_cap, d_boff, d_blen, tab, d_status, stream);
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_bgzf_close((uint8_t*)d_out, out_cap, d_boff + nb, 1u, d_out_len, d_status, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- writing ZIP archives (include/zmi355.h; the kernels: pack.hip, checksum.hip) ---------------------------------
// The pieces of all entries are one table of at most n_entries + in_bytes / piece_bytes places (the lengths live on the device: places
// behind the true count are void, length 0, and take no room in the archive).  The table goes through the independent-piece encoder in
// the launch groups of zmi_bgzf_body -- chain mode 2 with the bitmap of the pieces that end an entry's stream --, every group is placed
// behind the device word the group before ended at, so an entry may lie across groups; headers, directory and end structure are
// written once the last payload is in place.
extern "C" uint64_t zmi_zip_bound(uint32_t n_entries, uint64_t names_bytes, uint64_t in_bytes, uint32_t piece_bytes, int level) {
    if (piece_bytes == 0) return 0;
    // local header + central record with its ZIP64 extra + the name twice; the ZIP64 record, its locator, the end record
    uint64_t b = (uint64_t)n_entries * (30u + 46u + 12u) + 2u * names_bytes + 56u + 20u + 22u + in_bytes;
    if (level != 0) b += (in_bytes >> 3) + ((uint64_t)n_entries + in_bytes / piece_bytes) * 48u;   // zmi_deflate_pieces_stride per piece
    return b;
}

extern "C" int zmi_zip_write_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, uint64_t in_bytes,
                                 const void* d_names, const uint64_t* d_name_off, const uint32_t* d_dos_time, const uint32_t* d_ext_attr,
                                 uint32_t piece_bytes, int level, int strategy, uint64_t base, void* d_out, uint64_t out_cap,
                                 uint64_t* d_out_len, zmi_zip_entry* d_entries, zmi_zip_info* d_info, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    int rc = zmi_check_piece_bytes(piece_bytes);
    if (!rc) rc = zmi_check_level_strategy(level, strategy);
    if (rc) return rc;
    if (n > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "zmi_zip_write_dev: more than 2^31 - 1 entries");
    if (!d_out_len || !d_status || (out_cap && !d_out) || (n && (!d_in_off || !d_in_len || !d_name_off || (in_bytes && !d_in))))
        return zmi_fail(ZMI_E_ARG, "null argument");
    const uint64_t np64 = n ? (uint64_t)n + in_bytes / piece_bytes : 0u;
    if (np64 > 0x7FFFFFFFull) return zmi_fail(ZMI_E_ARG, "zmi_zip_write_dev: more than 2^31 - 1 pieces");
    const uint32_t np = (uint32_t)np64;
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);

    // A slot holds a piece of max_len = min(piece_bytes, in_bytes) bytes in the regions of a piece_bytes shard.  Level 0 has no slots:
    // the pieces are copied as they stand, in one group.  (No entries: no pieces, no group; what follows writes the end record alone.)
    const uint32_t max_len = in_bytes < piece_bytes ? (uint32_t)in_bytes : piece_bytes;
    uint64_t stride = 0;
    zmi_group_plan plan;
    if (level != 0) {
        stride = zmi_piece_slot_stride(max_len, piece_bytes, level);
        rc = zmi_plan_slots(c, np, max_len, stride, "scratch limit too small for one piece", &plan);
        if (rc) return rc;
    } else {
        plan = zmi_plan_groups_per(c->scratch_limit, zmi_group_override(), np, 0u);
    }
    const uint64_t group = plan.group;
    const uint32_t wpg = plan.wpg;
    const size_t bm_words = plan.bm_words;

    uint64_t *d_first, *d_coff, *d_poff, *d_pos;
    zmi_words4 neff;
    uint32_t *d_elen, *d_nlen, *d_npc, *d_ecrc, *d_csz, *d_plen, *d_head, *d_olen, *d_pcrc, *d_psz, *d_ends;
    int32_t* d_st;
    rc = zmi_carve(c->sd_meta, [&](zmi_carver k) {
        k.take(n + 1u, d_first, d_coff);                             // per entry: its first piece, its central record's offset
        k.take(np, d_poff);                                          // per piece: its place in d_in
        k.take(np + 1u, d_pos);                                      // ... and in the archive
        k.take(neff);                                                // the count that is listed; the sum of the checked lengths (u64)
        k.take(n, d_elen, d_nlen, d_npc, d_ecrc, d_csz);             // per entry: checked length, name length, pieces, CRC-32, central size
        k.take(np, d_plen, d_head, d_olen, d_st, d_pcrc, d_psz);     // per piece: length, hole, encoder's size and status, CRC-32, place's size
        k.take(bm_words, d_ends);                                    // the bitmap of the pieces that end an entry's stream
        k.skip(16u);                                                 // (spare: the reservation has always ended with it)
        return k.end();
    });
    if (rc) return rc;
    uint32_t* const d_neff = neff.w;
    uint64_t* const d_sum = neff.upper64();

    ZMI_HIP(hipMemsetAsync(d_status, 0, 4, stream));
    ZMI_HIP(hipMemsetAsync(d_pos, 0, 8, stream));     // where the first group's pack starts
    ZMI_HIP(hipMemsetAsync(d_neff, 0, 16, stream));
    if (bm_words) ZMI_HIP(hipMemsetAsync(d_ends, 0, bm_words * 4u, stream));
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_zip_layout(d_in_len, d_name_off, n, piece_bytes, d_elen, d_nlen, d_npc, d_sum, d_status, stream);
        zmi_launch_scan_sizes(d_npc, n, d_first, stream);
        zmi_launch_zip_pieces(d_in_off, d_elen, d_nlen, d_first, d_sum, n, in_bytes, piece_bytes, np, (uint32_t)group, wpg, d_poff, d_plen,
                              d_head, d_ends, d_neff, d_status, stream);
    }
    rc = zmi_piece_checks(c, d_in, d_poff, d_plen, np, ZMI_WRAP_GZIP, d_pcrc, stream);
    if (rc) return rc;
    for (uint64_t first = 0; first < np; first += group) {
        const uint32_t cnt = (uint32_t)(np - first < group ? np - first : group);
        if (level != 0) {
            rc = zmi_deflate_impl(c, {.d_in = d_in, .d_in_off = d_poff + first, .d_in_len = d_plen + first, .n = cnt, .max_len = max_len,
                                      .level = level, .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = 2u, .d_out = c->sd_slots.p,
                                      .out_stride = stride, .d_out_len = d_olen + first, .d_status = d_st + first, .stream = stream_, .carry = 0,
                                      .ends = d_ends + (first / group) * wpg, .geom_len = piece_bytes});
            if (rc) return rc;
        }
        // the group's pieces go behind the previous group's, the running offset never leaves the device
        const uint32_t* d_pay = level != 0 ? d_olen + first : d_plen + first;
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_zip_sizes(d_head + first, d_pay, level != 0 ? d_st + first : nullptr, cnt, d_psz + first, d_status, stream);
        zmi_launch_scan_sizes_base(d_psz + first, cnt, d_pos + first, d_pos + first, stream);
        zmi_launch_zip_pack((const uint8_t*)d_in, d_poff + first, d_head + first, level != 0 ? (const uint8_t*)c->sd_slots.p : nullptr, stride, d_pay,
                            cnt, level != 0 ? (stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride) : max_len, (uint8_t*)d_out, d_pos + first,
                            out_cap, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_combine_segments(d_pcrc, d_plen, d_first, n, d_neff, d_ecrc, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        const uint32_t method = level != 0 ? 8u : 0u;
        zmi_launch_zip_headers(d_elen, d_nlen, d_first, d_pos, d_ecrc, (const uint8_t*)d_names, d_name_off, d_dos_time, d_ext_attr, n, d_neff, method,
                               base, (uint8_t*)d_out, out_cap, d_csz, d_coff, nullptr, 0u, d_status, stream);
        zmi_launch_scan_sizes_base(d_csz, n, d_coff, d_pos + np, stream);
        zmi_launch_zip_headers(d_elen, d_nlen, d_first, d_pos, d_ecrc, (const uint8_t*)d_names, d_name_off, d_dos_time, d_ext_attr, n, d_neff, method,
                               base, (uint8_t*)d_out, out_cap, d_csz, d_coff, d_entries, 1u, d_status, stream);
        zmi_launch_zip_close((uint8_t*)d_out, out_cap, d_pos + np, d_coff + n, d_neff, base, d_out_len, d_info, d_status, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// The per-stream tables of one zmi_inflate_impl call in c->inf_tmp (32 bytes per stream): they stay valid on the stream until the next
// inflate call on the context.  check = the trailer's value, adler / crc = those of the produced bytes (zmi_inflate_members_dev reads
// them to tell a wrong CRC-32 from a wrong ISIZE).  This function is the one statement of the layout.
struct zmi_inf_tables { uint64_t* bm_off; uint32_t *used, *check, *adler, *crc, *order; };
static zmi_inf_tables zmi_inf_tables_of(zmi_ctx* c, uint32_t n) {
    zmi_inf_tables t;
    t.bm_off = (uint64_t*)c->inf_tmp.p;
    t.used = (uint32_t*)(t.bm_off + n);
    t.check = t.used + n;
    t.adler = t.check + n;
    t.crc = t.adler + n;
    t.order = t.crc + n;
    return t;
}
// What the core laid out for one launch, for the callers that go on with it (valid as the tables above): the bitmap, every stream's first
// word in it, and check / adler / crc (a resumable decode leaves the size of its last dynamic block's tables in `check`: inflateCodesUsed).
struct zmi_inf_scratch { const uint64_t *bitmap = nullptr, *bm_off = nullptr; const uint32_t *check = nullptr, *adler = nullptr, *crc = nullptr; };
// One call of the core; every call site names what it passes.  d_out_hist (may be null): per stream, the bytes directly in front of its
// output region that hold a preset dictionary (inflateSetDictionary, zlib-rs/src/inflate.rs:2492-2536; at most 32768 are ever referenced).
struct zmi_inf_req {
    const void* d_in = nullptr; const uint64_t* d_in_off = nullptr; const uint32_t* d_in_len = nullptr; uint32_t n = 0; int wrap = ZMI_WRAP_RAW;
    void* d_out = nullptr; const uint64_t* d_out_off = nullptr; const uint32_t *d_out_cap = nullptr, *d_out_hist = nullptr;   // the regions
    uint32_t* d_out_len = nullptr; int32_t* d_status = nullptr; uint32_t* d_in_used = nullptr; int32_t* d_detail = nullptr;   // the results
    const uint32_t* d_in_bit = nullptr; uint32_t* d_resume = nullptr;   // the resumable decode (zmi_inflate_resume_dev)
    void* stream = nullptr; const zmi_sd_inflate* sd = nullptr;
    bool decode_only = false;            // the caller resolves (it stitches the segments of one stream first)
    bool no_jump = false;                // never the jump resolve (a stream that is empty in all but a few calls)
    uint64_t out_limit = 0;              // output bytes the bitmap must cover; 0: the context's setting (zmi_ctx_set_inflate_out_limit)
    bool limit_exact = false;            // out_limit was sized from the capacities of THIS call
    zmi_inf_scratch* scratch = nullptr;  // (may be null) filled in for the caller
};
static int zmi_inflate_impl(zmi_ctx* c, const zmi_inf_req& q) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (q.wrap < ZMI_WRAP_RAW || q.wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    const uint32_t n = q.n;
    if (n == 0) return ZMI_E_OK;
    hipStream_t stream = (hipStream_t)q.stream;
    ZMI_ON_DEVICE(c);
    int rc = zmi_reserve(c->inf_tmp, (size_t)n * 32u);
    if (rc) return rc;
    const zmi_inf_tables tab = zmi_inf_tables_of(c, n);
    uint64_t* d_bm_off = tab.bm_off;
    uint32_t* d_used = tab.used;
    uint32_t* d_check = tab.check;
    uint32_t* d_adler = tab.adler;
    uint32_t* d_crc = tab.crc;
    uint32_t* d_order = tab.order;   // workgroup -> stream: largest compressed size first (zmi_inflate_order_kernel)
    if (q.d_in_used) d_used = q.d_in_used;
    const zmi_sd_inflate* const sd = q.sd;
    const uint32_t* d_out_hist = q.d_out_hist;
    if (sd) {   // the decode pass reads no history: all it needs is every stream's `hist` for its distance check and the FDICT branch
        uint32_t* d_hist = d_order + n;
        zmi_launch_inflate_shared_hist(d_hist, n, sd->hist, stream);
        d_out_hist = d_hist;
    }
    // bitmap scratch: 1 bit per byte of output capacity (+2 words per stream).  The capacities live on the
    // device, so the size comes from the caller's limit or the context's; streams beyond it report Z_MEM_ERROR.
    const uint64_t out_limit = q.out_limit ? q.out_limit : (c->inflate_out_limit ? c->inflate_out_limit : c->scratch_limit);
    rc = zmi_reserve(c->inf_bm, (size_t)(out_limit / 8u) + (size_t)n * 16u);
    if (rc) return rc;
    if (q.scratch) *q.scratch = {(const uint64_t*)c->inf_bm.p, d_bm_off, d_check, d_adler, d_crc};
    const uint64_t bm_words = ((out_limit / 8u) + (uint64_t)n * 16u) / 8u;
    uint32_t mw_max = c->inf_mw_max;
    if (const char* mv = zmi_tune("ZMI_INF_MW_MAX")) mw_max = (uint32_t)atoi(mv);   // (tests: both selections, per call)
    {
        zmi_scope_timer tm(c, ZMI_K_INFLATE, stream);
        int lrc = zmi_launch_inflate((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, n, (uint32_t)q.wrap, (uint8_t*)q.d_out, q.d_out_off, q.d_out_cap,
                                     q.d_out_len, d_used, d_check, q.d_status, (uint64_t*)c->inf_bm.p, bm_words, d_bm_off, d_out_hist, q.d_in_bit, q.d_resume,
                                     d_order, mw_max, stream);
        if (lrc) return zmi_fail(ZMI_E_HIP, "inflate launch setup", (hipError_t)lrc);
    }
    // The resolve pass.  Thousands of streams: one wave per stream fills its holes in order.  A handful of streams would leave
    // the chip empty that way (a 1 MiB stream alone: 8 ms): their back-references are resolved by pointer jumping over all
    // output bytes at once (resolve_jump.hip), which costs 4 B of scratch per byte of capacity.
    // (below 256 KiB of capacity the serial pass takes less than the jump pass's two dozen launches)
    // (the pass sweeps out_limit indices whatever the streams' real capacities are -- they are device data: a limit far above what n
    // streams plausibly hold, 64 MiB each, says the caller did not size it for this call, and the serial pass is the safer choice)
    // (limit_exact, callers that sized the limit from this call's capacities -- zmi_inflate_resume, the packed calls, the plain host-buffer
    // batch; not the pipelined one, sized once for its largest chunk: one stream of several hundred MiB keeps the jump pass)
    // (round 6: ONE stream under an exact limit -- a streaming inflate() of the zlib ABI, zmi_inflate_resume -- always takes the jump pass
    // (an exact limit is a capacity plus 64 KiB or more: jump_min never filters it): its serial pass is one wave alone on the chip, 389 us
    // for the ~40 KiB of an open block, against a dozen launches of a few microseconds; the reference's chunk sweep at 1 / 4 / 16 / 64 KiB
    // pieces: 0.90 / 0.248 / 0.069 / 0.020 s -> 0.59 / 0.153 / 0.046 / 0.018 s for 4 MiB, profiles/r06_eager_inflate_trace.txt)
    const uint64_t jump_min = (n == 1u && q.limit_exact) ? (64ull << 10) : (256ull << 10);
    bool jump = n <= 16u && out_limit <= (1ull << 30) && out_limit >= jump_min &&
                (q.limit_exact || out_limit <= (uint64_t)n * (64ull << 20) + (1ull << 20));
    if (!q.decode_only) {
    if (const char* jv = zmi_tune("ZMI_INF_JUMP")) jump = atoi(jv) != 0 && out_limit <= (1ull << 30);
    if (q.no_jump) jump = false;   // (the caller's stream is empty in all but a few calls: the jump resolve would sweep the limit for nothing)
    if (sd) jump = false;   // the shared dictionary is read by the one-wave-per-stream pass only (its case is many small streams)
    if (jump && zmi_reserve(c->inf_ptr, (size_t)bm_words * 256u + 512u) != 0) jump = false;   // (no room: the serial pass needs none)
    {
        zmi_scope_timer tm(c, ZMI_K_RESOLVE, stream);
        int lrc;
        if (jump) {
            uint32_t rounds = 2u;   // ceil(log3(capacity)) + 1: a round follows two pointers (resolve_jump.hip)
            for (uint64_t span = 3u; rounds < 34u && span < out_limit; span *= 3u) ++rounds;
            lrc = zmi_launch_resolve_jump((uint8_t*)q.d_out, q.d_out_off, q.d_out_len, n, (const uint64_t*)c->inf_bm.p, d_bm_off, (int32_t*)c->inf_ptr.p,
                                          bm_words * 64ull, rounds, (uint32_t*)((uint8_t*)c->inf_ptr.p + (size_t)bm_words * 256u), stream);
        } else if (sd) {
            lrc = zmi_launch_inflate_resolve_shared((uint8_t*)q.d_out, q.d_out_off, q.d_out_len, n, (const uint64_t*)c->inf_bm.p, d_bm_off, d_order,
                                                    sd->img, sd->hist, stream);
        } else {
            lrc = zmi_launch_inflate_resolve((uint8_t*)q.d_out, q.d_out_off, q.d_out_len, n, (const uint64_t*)c->inf_bm.p, d_bm_off, d_out_hist, d_order, stream);
        }
        if (lrc) return zmi_fail(ZMI_E_HIP, "inflate resolve launch setup", (hipError_t)lrc);
    }
    }   // (decode_only: the caller resolves -- zmi_inflate_split stitches the segments of one stream first)
    if (q.wrap != ZMI_WRAP_RAW) {
        uint32_t kind = q.wrap == ZMI_WRAP_ZLIB ? 1u : (q.wrap == ZMI_WRAP_GZIP ? 2u : 3u);
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_checksum((const uint8_t*)q.d_out, q.d_out_off, q.d_out_len, n, kind, d_adler, d_crc, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_inflate_verify((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, n, (uint32_t)q.wrap, d_check, d_adler, d_crc, q.d_status,
                                  q.d_detail, stream);
        // inflateSetDictionary refuses a dictionary whose Adler-32 is not the stream's DICTID (inflate.rs:2492-2536)
        if (sd && q.wrap == ZMI_WRAP_ZLIB)
            zmi_launch_inflate_dictid((const uint8_t*)q.d_in, q.d_in_off, q.d_in_len, n, sd->dictid, q.d_status, q.d_detail, q.d_out_len, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// The request with one preset dictionary for all its streams (dict_len > 0, n > 0, wrap raw or zlib: the callers saw to that).
static int zmi_inflate_shared_dict(zmi_ctx* c, zmi_inf_req q, const void* d_dict, uint32_t dict_len) {
    zmi_sd_inflate sd;
    {
        ZMI_ON_DEVICE(c);
        const uint32_t hist = dict_len < 32768u ? dict_len : 32768u;
        const uint32_t shift = (hist + 1023u) & ~1023u;   // the resolve pass's staging block (RES_BLK, inflate.hip)
        int rc = zmi_sd_prepare(c, d_dict, dict_len, true, q.wrap == ZMI_WRAP_ZLIB, (hipStream_t)q.stream, shift - hist, hist, 32u);
        if (rc) return rc;
        sd.img = (const uint8_t*)c->dict.p + ZMI_SD_INF_IMG;
        sd.hist = hist;
        sd.dictid = (const uint32_t*)((const uint8_t*)c->dict.p + ZMI_SD_DICTID);
    }
    q.sd = &sd;
    return zmi_inflate_impl(c, q);
}

// Every stream as inflateInit2_ + inflateSetDictionary(dict) + inflate(Z_FINISH), one dictionary for the whole call; see
// include/zmi355.h.
extern "C" int zmi_inflate_batch_shared_dict_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                 uint32_t n, int wrap, const void* d_dict, uint32_t dict_len, void* d_out,
                                                 const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                                                 int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap != ZMI_WRAP_RAW && wrap != ZMI_WRAP_ZLIB) return zmi_fail(ZMI_E_ARG, "a preset dictionary needs wrap raw or zlib (a gzip member has no dictionary field)");
    const zmi_inf_req q{.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .wrap = wrap, .d_out = d_out, .d_out_off = d_out_off,
                        .d_out_cap = d_out_cap, .d_out_len = d_out_len, .d_status = d_status, .d_in_used = d_in_used, .d_detail = d_detail,
                        .stream = stream_};
    if (!d_dict || dict_len == 0u || n == 0u) return zmi_inflate_impl(c, q);
    return zmi_inflate_shared_dict(c, q, d_dict, dict_len);
}

// extended forms used by the zlib stream ABI: also return consumed input bytes and why a stream stopped
extern "C" int zmi_inflate_batch_dict_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                          uint32_t n, int wrap, void* d_out, const uint64_t* d_out_off,
                                          const uint32_t* d_out_cap, const uint32_t* d_out_hist, uint32_t* d_out_len,
                                          int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream_) {
    return zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .wrap = wrap, .d_out = d_out,
                                .d_out_off = d_out_off, .d_out_cap = d_out_cap, .d_out_hist = d_out_hist, .d_out_len = d_out_len,
                                .d_status = d_status, .d_in_used = d_in_used, .d_detail = d_detail, .stream = stream_});
}
extern "C" int zmi_inflate_batch_dev_ex(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                        uint32_t n, int wrap, void* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                        uint32_t* d_out_len, int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail,
                                        void* stream_) {
    return zmi_inflate_batch_dict_dev(c, d_in, d_in_off, d_in_len, n, wrap, d_out, d_out_off, d_out_cap, nullptr, d_out_len,
                                      d_status, d_in_used, d_detail, stream_);
}

// Resumable raw-deflate decode (the device half of a streaming inflate; the facts the reference keeps in
// Mode / BitReader / Window, zlib-rs/src/inflate.rs:288-320, reduced to a block-boundary checkpoint).
// Stream i starts at bit d_in_bit[i] (0..7; array may be NULL) of its first byte, with d_out_hist[i] bytes of
// earlier output in front of its output region.  d_resume[4i..4i+3] = {byte, bit, output bytes, complete}: the
// start of the block the decode stopped in (status Z_BUF_ERROR: more input or more room needed), or the first bit
// behind the final block (complete = 1).  d_out_len[i] counts everything decoded, also the valid part of the
// unfinished block; a later call that starts at the checkpoint reproduces those bytes and continues.
extern "C" int zmi_inflate_resume_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                      const uint32_t* d_in_bit, uint32_t n, void* d_out, const uint64_t* d_out_off,
                                      const uint32_t* d_out_cap, const uint32_t* d_out_hist, uint32_t* d_out_len,
                                      int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, uint32_t* d_resume,
                                      void* stream_) {
    if (!d_resume) return zmi_fail(ZMI_E_ARG, "d_resume is required");
    return zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .wrap = ZMI_WRAP_RAW, .d_out = d_out,
                                .d_out_off = d_out_off, .d_out_cap = d_out_cap, .d_out_hist = d_out_hist, .d_out_len = d_out_len, .d_status = d_status,
                                .d_in_used = d_in_used, .d_detail = d_detail, .d_in_bit = d_in_bit, .d_resume = d_resume, .stream = stream_});
}

extern "C" int zmi_inflate_batch_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                     uint32_t n, int wrap, void* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                     uint32_t* d_out_len, int32_t* d_status, void* stream_) {
    return zmi_inflate_batch_dev_ex(c, d_in, d_in_off, d_in_len, n, wrap, d_out, d_out_off, d_out_cap, d_out_len, d_status, nullptr,
                                    nullptr, stream_);
}

// ---- batch inflate without an output size table (include/zmi355.h) ----
// The size pass: the decode kernel's SIZE form (inflate.hip).  Of the context's inf_tmp tables it uses `order` (and `used` when the
// caller wants no d_in_used); it needs no bitmap.
static int zmi_inflate_sizes_impl(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, int wrap,
                                  uint32_t hist, uint32_t size_limit, uint32_t* d_size, int32_t* d_status, uint32_t* d_in_used,
                                  int32_t* d_detail, hipStream_t stream) {
    int rc = zmi_reserve(c->inf_tmp, (size_t)n * 32u);
    if (rc) return rc;
    const zmi_inf_tables tab = zmi_inf_tables_of(c, n);
    uint32_t mw_max = c->inf_mw_max;
    if (const char* mv = zmi_tune("ZMI_INF_MW_MAX")) mw_max = (uint32_t)atoi(mv);   // (tests: both selections, per call)
    zmi_scope_timer tm(c, ZMI_K_INFLATE, stream);
    int lrc = zmi_launch_inflate_sizes((const uint8_t*)d_in, d_in_off, d_in_len, n, (uint32_t)wrap, hist, size_limit ? size_limit : 0xFFFFFFFFu,
                                       d_size, d_status, d_in_used, d_detail, tab.order, mw_max, stream);
    if (lrc) return zmi_fail(ZMI_E_HIP, "inflate size pass launch setup", (hipError_t)lrc);
    return ZMI_E_OK;
}

extern "C" int zmi_inflate_sizes_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                     int wrap, uint32_t hist, uint32_t size_limit, uint32_t* d_size, int32_t* d_status,
                                     uint32_t* d_in_used, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    if (hist > 32768u) return zmi_fail(ZMI_E_ARG, "hist must be 0 .. 32768");
    if (n == 0) return ZMI_E_OK;
    if (!d_size || !d_status) return zmi_fail(ZMI_E_ARG, "d_size and d_status are required");
    ZMI_ON_DEVICE(c);
    int rc = zmi_inflate_sizes_impl(c, d_in, d_in_off, d_in_len, n, wrap, hist, size_limit, d_size, d_status, d_in_used, d_detail,
                                    (hipStream_t)stream_);
    if (rc) return rc;
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// What the packed call does behind its size pass, shared with zmi_zip_inflate_dev (which takes the sizes from the directory): the plan
// -- d_out_off, and d_cap[i] = d_size[i] where the region ends at or before out_cap, else 0 -- the decode with the planned tables under
// a bitmap sized from out_cap, and the mark of the streams that did not fit.  plan_timer: the event-timing slot of the plan, -1 none.
static int zmi_inflate_packed_body(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, int wrap,
                                   const void* d_dict, uint32_t dict_len, const uint32_t* d_size, uint32_t* d_cap, uint32_t out_align,
                                   void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status,
                                   uint32_t* d_in_used, int32_t* d_detail, int plan_timer, void* stream_, const uint32_t* d_want = nullptr,
                                   uint32_t* d_dcap = nullptr) {
    hipStream_t stream = (hipStream_t)stream_;
    if (plan_timer >= 0) {
        zmi_scope_timer tm(c, plan_timer, stream);
        zmi_launch_inflate_pack_plan(d_size, n, out_align, out_cap, d_out_off, d_cap, stream);
    } else {
        zmi_launch_inflate_pack_plan(d_size, n, out_align, out_cap, d_out_off, d_cap, stream);
    }
    // d_want (zmi_exr_read_dev): a stream must give d_want[i] <= d_size[i] bytes; its room stays the plan's
    if (d_want) zmi_launch_exr_deccap(d_size, d_cap, d_want, n, d_dcap, stream);
    // the bitmap scratch covers what the planned capacities can sum to: out_cap (no stream holds more than 2^32 - 1 bytes)
    const uint64_t most = (uint64_t)n * 0xFFFFFFFFull;
    const zmi_inf_req q{.d_in = d_in, .d_in_off = d_in_off, .d_in_len = d_in_len, .n = n, .wrap = wrap, .d_out = d_out, .d_out_off = d_out_off,
                        .d_out_cap = d_want ? d_dcap : d_cap, .d_out_len = d_out_len, .d_status = d_status, .d_in_used = d_in_used, .d_detail = d_detail,
                        .stream = stream_, .out_limit = (out_cap < most ? out_cap : most) + (1ull << 16), .limit_exact = true};
    const int rc = d_dict ? zmi_inflate_shared_dict(c, q, d_dict, dict_len) : zmi_inflate_impl(c, q);
    if (rc) return rc;
    zmi_launch_inflate_pack_mark(d_size, d_out_off, n, out_cap, d_out_len, d_status, d_in_used, d_detail, stream);
    return ZMI_E_OK;
}

extern "C" int zmi_inflate_batch_packed_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                            int wrap, const void* d_dict, uint32_t dict_len, uint32_t size_limit, uint32_t out_align,
                                            void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status,
                                            uint32_t* d_in_used, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    int rc = zmi_check_out_align(out_align);
    if (rc) return rc;
    const bool dict = d_dict != nullptr && dict_len != 0u;
    if (dict && wrap != ZMI_WRAP_RAW && wrap != ZMI_WRAP_ZLIB)
        return zmi_fail(ZMI_E_ARG, "a preset dictionary needs wrap raw or zlib (a gzip member has no dictionary field)");
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    if (n == 0) {
        ZMI_HIP(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), stream));
        return ZMI_E_OK;
    }
    if (!d_out_len || !d_status) return zmi_fail(ZMI_E_ARG, "d_out_len and d_status are required");
    rc = zmi_reserve(c->pk, (size_t)n * 8u);
    if (rc) return rc;
    uint32_t* d_size = (uint32_t*)c->pk.p;
    uint32_t* d_cap = d_size + n;
    // (the size pass leaves its words in the caller's arrays; the decode below overwrites them)
    rc = zmi_inflate_sizes_impl(c, d_in, d_in_off, d_in_len, n, wrap, dict ? (dict_len < 32768u ? dict_len : 32768u) : 0u, size_limit, d_size,
                                d_status, d_in_used, d_detail, stream);
    if (rc) return rc;
    rc = zmi_inflate_packed_body(c, d_in, d_in_off, d_in_len, n, wrap, dict ? d_dict : nullptr, dict_len, d_size, d_cap, out_align, d_out, out_cap,
                                 d_out_off, d_out_len, d_status, d_in_used, d_detail, -1, stream_);
    if (rc) return rc;
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- ZIP archives (include/zmi355.h; kernels in pack.hip) ----
extern "C" int zmi_zip_directory_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, zmi_zip_entry* d_entries, uint32_t cap, zmi_zip_info* d_info,
                                     void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (!d_info || (in_len && !d_in) || (cap && !d_entries)) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    const uint64_t nseg = zmi_zip_segments(in_len);
    int rc = zmi_reserve(c->zip_dir, 32u + (size_t)cap * 8u + (size_t)nseg * 32u);
    if (rc) return rc;
    uint32_t stages = 3u;
    if (const char* sv = zmi_tune("ZMI_ZIP_STAGES")) stages = (uint32_t)atoi(sv);   // (the probe: locate / walk / parse timed apart)
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        uint64_t* d_w = (uint64_t*)c->zip_dir.p;
        zmi_launch_zip_directory((const uint8_t*)d_in, in_len, d_entries, cap, d_info, d_w, d_w + 4, d_w + 4 + cap, stages, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_zip_inflate_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, const zmi_zip_entry* d_entries, uint32_t n_entries,
                                   const uint32_t* d_sel, uint32_t n_sel, uint32_t out_align, void* d_out, uint64_t out_cap,
                                   uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    int rc = zmi_check_out_align(out_align);
    if (rc) return rc;
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    bool done;
    rc = zmi_empty_selection(n_sel, d_out_off, d_out_len, d_status, d_detail, stream, &done);
    if (rc || done) return rc;
    if ((n_entries && !d_entries) || (in_len && !d_in) || (out_cap && !d_out)) return zmi_fail(ZMI_E_ARG, "null argument");
    uint64_t* d_in_off;
    uint32_t *d_in_n, *d_size, *d_slen, *d_cap, *d_used, *d_crc;
    rc = zmi_carve(c->zip_sel, [&](zmi_carver k) {
        k.take(n_sel, d_in_off);     // the entry's first data byte
        k.take(n_sel, d_in_n);       // csize of a deflated slot, 0 for every other
        k.take(n_sel, d_size);       // usize of a readable slot: the plan's sizes
        k.take(n_sel, d_slen);       // usize of a stored slot: the copy's lengths
        k.take(n_sel, d_cap);        // the planned size where the region fits out_cap, else 0
        k.take(n_sel, d_used, d_crc);
        return k.end();
    });
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_zip_prep(d_entries, n_entries, d_sel, n_sel, in_len, d_in_off, d_in_n, d_size, d_slen, stream);
    }
    rc = zmi_inflate_packed_body(c, d_in, d_in_off, d_in_n, n_sel, ZMI_WRAP_RAW, nullptr, 0u, d_size, d_cap, out_align, d_out, out_cap, d_out_off,
                                 d_out_len, d_status, d_used, d_detail, ZMI_K_PARSE, stream_);
    if (rc) return rc;
    {
        // stored slots: a range that would end behind out_cap is skipped by the copy itself; max_len only shapes the launch
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_copy_ranges((const uint8_t*)d_in, d_in_off, 0u, d_slen, n_sel, (uint8_t*)d_out, d_out_off, out_cap,
                               in_len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)in_len, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_checksum((const uint8_t*)d_out, d_out_off, d_cap, n_sel, 2u, nullptr, d_crc, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_zip_verify(d_entries, n_entries, d_sel, n_sel, in_len, d_out_off, out_cap, d_used, d_crc, d_out_len, d_status, d_detail, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- PNG images (include/zmi355.h; kernels in png_kernels.h) ----
extern "C" int zmi_png_headers_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_images,
                                   zmi_png_image* d_images, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (n_images == 0) return ZMI_E_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_images) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_png_headers((const uint8_t*)d_in, d_in_off, d_in_len, n_images, d_images, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_png_decode_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_png_image* d_images,
                                  uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, uint32_t flags, uint32_t out_align, void* d_out,
                                  uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    int rc = zmi_check_out_align(out_align);
    if (rc) return rc;
    if (flags & ~(ZMI_PNG_NATIVE16 | ZMI_PNG_NO_CRC)) return zmi_fail(ZMI_E_ARG, "unknown flag");
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    if (n_sel > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "n_sel must be below 2^31");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    bool done;
    rc = zmi_empty_selection(n_sel, d_out_off, d_out_len, d_status, d_detail, stream, &done);
    if (rc || done) return rc;
    if ((n_images && (!d_images || !d_in || !d_in_off || !d_in_len)) || (out_cap && !d_out)) return zmi_fail(ZMI_E_ARG, "null argument");
    if (out_cap > (1ull << 44)) return zmi_fail(ZMI_E_NOMEM, "out_cap sizes the scratch: give the room there is");
    // Everything is sized from out_cap and n_sel: no size of the input is known here.  Scanlines: 1 + row_bytes <= 2 * row_bytes, and
    // every region starts at a multiple of 16.  Gathered streams: see the header.
    const size_t n = n_sel;
    const uint64_t scan_cap = 2ull * out_cap + 16ull * n + 64ull;
    // (the gather buffer is this call's own addition to what the decoder needs: it stays under the context's scratch limit)
    uint64_t gather_cap = 2ull * out_cap + (out_cap >> 3) + 1024ull * n + (64ull << 10);
    if (gather_cap > c->scratch_limit) gather_cap = c->scratch_limit;
    uint64_t *d_goff, *d_soff, *d_item_off, *d_zin_off;
    uint32_t *d_pix, *d_pcap, *d_ssz, *d_scap, *d_gsz, *d_gcap, *d_items, *d_fl, *d_zin_len, *d_slen, *d_sused;
    int32_t *d_sst, *d_sdet;
    uint8_t *d_gbuf, *d_sbuf;
    rc = zmi_carve(c->png, [&](zmi_carver k) {
        k.take(n + 1, d_goff);           // where the gathered stream of a slot stands (the plan over d_gsz)
        k.take(n + 1, d_soff);           // ... its filtered scanlines (the decoder's own plan over d_ssz)
        k.take(n + 1, d_item_off);       // the scan of d_items
        k.take(n, d_zin_off);            // where the decoder reads the slot's zlib stream
        k.take(n, d_pix);                // height * row_bytes of a readable slot, else 0
        k.take(n, d_pcap);               // ... where the region fits out_cap, else 0
        k.take(n, d_ssz, d_scap);        // (1 + row_bytes) * height of a slot that is decoded, else 0; its planned capacity
        k.take(n, d_gsz, d_gcap);        // idat_bytes of a decoded slot with several IDAT chunks, else 0; its planned capacity
        k.take(n, d_items);              // bands of 64 rows
        k.take(n, d_fl, d_zin_len);      // PNG_FL_*: set by the walk and the unfilter; the zlib stream's length
        k.take(n, d_slen, d_sused, d_sst, d_sdet);   // the decoder's words
        k.align(256u);
        k.take(gather_cap, d_gbuf);      // the gathered streams
        k.skip(16u);
        k.align(256u);
        k.region(d_sbuf, scan_cap, 16u); // the filtered scanlines (the unfilter reads whole dwords around a row: 16 bytes of margin)
        return k.end();
    });
    if (rc) return rc;
    uint32_t split = 1u;
    if (const char* sv = zmi_tune("ZMI_PNG_SPLIT")) split = (uint32_t)atoi(sv);   // (the probe: a chain per image instead of per None / Sub row)
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_png_prep(d_images, n_images, d_sel, n_sel, d_in_len, 0u, d_pix, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
        zmi_launch_inflate_pack_plan(d_pix, n_sel, out_align, out_cap, d_out_off, d_pcap, stream);
        zmi_launch_png_prep(d_images, n_images, d_sel, n_sel, d_in_len, 1u, d_pix, d_pcap, d_ssz, d_gsz, d_items, d_fl, stream);
        zmi_launch_inflate_pack_plan(d_gsz, n_sel, 16u, gather_cap, d_goff, d_gcap, stream);
        zmi_launch_scan_sizes(d_items, n_sel, d_item_off, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_png_walk((const uint8_t*)d_in, d_in_off, d_in_len, d_images, d_sel, n_sel, d_ssz, d_gsz, d_goff, d_gcap, d_gbuf,
                            (flags & ZMI_PNG_NO_CRC) ? 0u : 1u, d_zin_off, d_zin_len, d_fl, stream);
    }
    rc = zmi_inflate_packed_body(c, d_in, d_zin_off, d_zin_len, n_sel, ZMI_WRAP_ZLIB, nullptr, 0u, d_ssz, d_scap, 16u, d_sbuf, scan_cap, d_soff,
                                 d_slen, d_sst, d_sused, d_sdet, ZMI_K_PARSE, stream_);
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_ENCODE, stream);
        zmi_launch_png_unfilter(d_images, d_sel, n_sel, d_item_off, out_cap / 64u + n, d_sbuf, d_soff, d_ssz, d_slen, d_sst, (uint8_t*)d_out,
                                d_out_off, (flags & ZMI_PNG_NATIVE16) ? 1u : 0u, split, d_fl, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_png_finish(d_images, n_images, d_sel, n_sel, d_in_len, d_out_off, out_cap, d_ssz, d_slen, d_sst, d_fl, d_out_len, d_status,
                              d_detail, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- TIFF files (include/zmi355.h; kernels in tiff_kernels.h) -------------------------------------------------------
extern "C" int zmi_tiff_directory_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, zmi_tiff_page* d_pages, uint32_t cap, zmi_tiff_info* d_info,
                                      void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (!d_info || (in_len && !d_in) || (cap && !d_pages)) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    int rc = zmi_reserve(c->tiff_dir, 64u + (size_t)cap * 8u);
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_tiff_directory((const uint8_t*)d_in, in_len, d_pages, cap, d_info, (uint64_t*)c->tiff_dir.p, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_tiff_read_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page,
                                 const uint32_t* d_sel, uint32_t n_sel, uint64_t decoded_bytes, uint32_t flags, uint32_t out_align, void* d_out,
                                 uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (flags & ~ZMI_TIFF_ASSEMBLE) return zmi_fail(ZMI_E_ARG, "unknown flag");
    const uint32_t assemble = (flags & ZMI_TIFF_ASSEMBLE) ? 1u : 0u;
    int rc = assemble ? ZMI_E_OK : zmi_check_out_align(out_align);
    if (rc) return rc;
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    if (n_sel > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "n_sel must be below 2^31");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    bool done;
    rc = zmi_empty_selection(n_sel, d_out_off, d_out_len, d_status, d_detail, stream, &done);
    if (rc || done) return rc;
    if ((n_pages && !d_pages) || (in_len && !d_in) || (out_cap && !d_out)) return zmi_fail(ZMI_E_ARG, "null argument");
    if (decoded_bytes > (1ull << 44)) return zmi_fail(ZMI_E_NOMEM, "decoded_bytes sizes the scratch: give the sum there is");
    // The still-predicted segments stand in scratch, every one at a multiple of 16 (the decoder's own plan over d_ssz), 16 bytes of
    // margin on either side: the unpredict stages whole dwords around a row.
    const size_t n = n_sel;
    const uint64_t scan_cap = decoded_bytes + 16ull * n + 64ull;
    uint64_t *d_soff, *d_item_off, *d_pix_off, *d_zin_off;
    uint32_t *d_pix, *d_pcap, *d_ssz, *d_scap, *d_zin_len, *d_rawlen, *d_items, *d_fl, *d_slen, *d_sused;
    int32_t *d_sst, *d_sdet;
    uint8_t* d_sbuf;
    rc = zmi_carve(c->tiff, [&](zmi_carver k) {
        k.take(n + 1, d_soff);           // where the segment of a slot stands in scratch (the decoder's plan over d_ssz)
        k.take(n + 1, d_item_off);       // the scan of d_items
        k.take(n + 1, d_pix_off);        // the scan of d_pix: its last word is the sum decoded_bytes bounds
        k.take(n, d_zin_off);            // the segment's place in the file
        k.take(n, d_pix);                // the decoded size of a slot that reads a segment, else 0
        k.take(n, d_pcap);               // ... where its region fits out_cap, else 0
        k.take(n, d_ssz, d_scap);        // ... where its bytes are fetched: not sparse, inside the file; its planned capacity
        k.take(n, d_zin_len);            // the byte count of a deflated slot
        k.take(n, d_rawlen);             // the bytes to copy for a slot of compression 1
        k.take(n, d_items);              // groups of TIFF_ROWS rows
        k.take(n, d_fl);                 // TIFF_FL_*
        k.take(n, d_slen, d_sused, d_sst, d_sdet);   // the decoder's words
        k.skip(8u * n);                  // (spare: the reservation has always counted two tables more than there are)
        k.align(256u);
        k.region(d_sbuf, scan_cap, 16u); // the still-predicted segments
        return k.end();
    });
    if (rc) return rc;
    const uint8_t* in = (const uint8_t*)d_in;
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_tiff_slots(in, in_len, d_pages, n_pages, page, d_sel, n_sel, assemble, 0u, out_cap, decoded_bytes, nullptr, d_pix, d_pcap, d_zin_off,
                              d_zin_len, nullptr, nullptr, nullptr, d_fl, d_out_off, stream);
        if (!assemble) zmi_launch_inflate_pack_plan(d_pix, n_sel, out_align, out_cap, d_out_off, d_pcap, stream);
        zmi_launch_scan_sizes(d_pix, n_sel, d_pix_off, stream);
        zmi_launch_tiff_slots(in, in_len, d_pages, n_pages, page, d_sel, n_sel, assemble, 1u, out_cap, decoded_bytes, d_pix_off, d_pix, d_pcap,
                              d_zin_off, d_zin_len, d_ssz, d_rawlen, d_items, d_fl, d_out_off, stream);
        zmi_launch_scan_sizes(d_items, n_sel, d_item_off, stream);
    }
    rc = zmi_inflate_packed_body(c, d_in, d_zin_off, d_zin_len, n_sel, ZMI_WRAP_ZLIB, nullptr, 0u, d_ssz, d_scap, 16u, d_sbuf, scan_cap, d_soff,
                                 d_slen, d_sst, d_sused, d_sdet, ZMI_K_PARSE, stream_);
    if (rc) return rc;
    {
        // compression 1: the segment's bytes as they stand (max_len only shapes the launch)
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_copy_ranges(in, d_zin_off, 0u, d_rawlen, n_sel, d_sbuf, d_soff, scan_cap, in_len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)in_len,
                               stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_ENCODE, stream);
        zmi_launch_tiff_unpredict(d_pages, n_pages, page, d_sel, n_sel, in_len, assemble, d_item_off, decoded_bytes / 8u + n, d_sbuf, d_soff, d_ssz,
                                  d_slen, d_sst, d_rawlen, d_fl, (uint8_t*)d_out, d_out_off, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_tiff_finish(d_pages, n_pages, page, d_sel, n_sel, in_len, assemble, out_cap, decoded_bytes, d_pix_off, d_out_off, d_ssz, d_slen,
                               d_sst, d_fl, d_out_len, d_status, d_detail, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- OpenEXR images (include/zmi355.h; kernels in exr_kernels.h) ----------------------------------------------------
extern "C" int zmi_exr_headers_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_files,
                                   zmi_exr_image* d_images, zmi_exr_channel* d_channels, uint32_t chan_cap, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (n_files == 0) return ZMI_E_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_images || (chan_cap && !d_channels)) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_exr_headers((const uint8_t*)d_in, d_in_off, d_in_len, n_files, d_images, d_channels, chan_cap, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_exr_read_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_exr_image* d_images,
                                const zmi_exr_channel* d_channels, uint32_t chan_cap, uint32_t n_files, const uint32_t* d_sel, uint32_t n_sel,
                                uint32_t chunk_cap, uint64_t decoded_bytes, uint32_t flags, uint32_t out_align, void* d_out, uint64_t out_cap,
                                uint64_t* d_out_off, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (flags != 0u) return zmi_fail(ZMI_E_ARG, "unknown flag");
    int rc = zmi_check_out_align(out_align);
    if (rc) return rc;
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    if (n_sel > 0x7FFFFFFFu || chunk_cap > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "n_sel and chunk_cap must be below 2^31");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    bool done;
    rc = zmi_empty_selection(n_sel, d_out_off, d_out_len, d_status, d_detail, stream, &done);
    if (rc || done) return rc;
    if ((n_files && (!d_images || !d_channels || !d_in || !d_in_off || !d_in_len)) || (out_cap && !d_out)) return zmi_fail(ZMI_E_ARG, "null argument");
    if (decoded_bytes > (1ull << 40)) return zmi_fail(ZMI_E_NOMEM, "decoded_bytes sizes the scratch: give the sum there is");
    // The inflated chunks stand in scratch, every one at a multiple of 16 (the decoder's own plan over d_csz), 16 bytes of margin at
    // either end of the scratch: the unzip loads whole dwords around a stream and whole 16-byte lines for its carries.
    const size_t n = n_sel, cc = chunk_cap;
    const uint64_t nblk = decoded_bytes / 1024u + cc;                 // (EXR_BLOCK: every chunk ends with at most one short block)
    const uint64_t scan_cap = decoded_bytes + 16ull * cc + 64ull;
    uint64_t *d_ch_off, *d_raw_off, *d_soff, *d_item_off, *d_blk_off, *d_zin_off, *d_pitem_off;
    uint32_t *d_size, *d_pcap, *d_nch, *d_rawb, *d_kind, *d_live;
    uint32_t *d_zin_len, *d_csz, *d_scap, *d_rawlen, *d_fl, *d_items, *d_nblk, *d_cslot, *d_slen, *d_sused, *d_bsum, *d_bpre, *d_cm, *d_pitems, *d_dcap;
    int32_t *d_sst, *d_sdet;
    uint8_t* d_sbuf;
    rc = zmi_carve(c->exr, [&](zmi_carver k) {
        k.take(n + 1, d_ch_off);         // the scan of d_nch: the chunks of slot j are d_ch_off[j] .. d_ch_off[j + 1)
        k.take(n + 1, d_raw_off);        // the scan of d_rawb: what decoded_bytes bounds
        k.take(cc + 1, d_soff);          // where a chunk stands in scratch (the decoder's plan over d_csz)
        k.take(cc + 1, d_item_off);      // the scan of d_items
        k.take(cc + 1, d_blk_off);       // the scan of d_nblk
        k.take(cc + 1, d_zin_off);       // the chunk's data in d_in
        k.take(cc + 1, d_pitem_off);     // the scan of d_pitems
        k.take(n, d_size);               // per slot: the region of a readable file, else 0
        k.take(n, d_pcap);               // ... where it fits out_cap, else 0
        k.take(n, d_nch);                // its chunks
        k.take(n, d_rawb);               // its raw bytes
        k.take(n, d_kind, d_live);
        k.take(cc, d_zin_len);           // per chunk: dataSize of a compressed chunk
        k.take(cc, d_csz, d_scap);       // the raw size n of a chunk whose header is right; its planned capacity
        k.take(cc, d_rawlen);            // n of a chunk stored raw: the copy's length
        k.take(cc, d_fl);                // EXR_FL_*
        k.take(cc, d_items);             // the pieces of the chunk's runs
        k.take(cc, d_nblk);              // the blocks of byte sums of a compressed chunk
        k.take(cc, d_cslot);             // the chunk's slot
        k.take(cc, d_cm, d_dcap);        // the bytes its stream must inflate to (PXR24: m < n); the decoder's capacity
        k.take(cc, d_pitems);            // the runs of a PXR24 stream
        k.take(cc, d_slen, d_sused, d_sst, d_sdet);   // the decoder's words
        k.take(nblk, d_bsum);            // one byte sum per block
        k.take(nblk, d_bpre);            // ... and the sums in front of it inside its chunk
        k.align(256u);
        k.region(d_sbuf, scan_cap, 16u); // the inflated chunks
        return k.end();
    });
    if (rc) return rc;
    const uint8_t* in = (const uint8_t*)d_in;
    {
        zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
        zmi_launch_exr_slots(d_in_len, d_images, d_channels, chan_cap, n_files, d_sel, n_sel, 0u, chunk_cap, decoded_bytes, nullptr, nullptr, nullptr,
                             d_size, d_nch, d_rawb, d_kind, d_live, stream);
        zmi_launch_inflate_pack_plan(d_size, n_sel, out_align, out_cap, d_out_off, d_pcap, stream);
        zmi_launch_scan_sizes(d_nch, n_sel, d_ch_off, stream);
        zmi_launch_scan_sizes(d_rawb, n_sel, d_raw_off, stream);
        zmi_launch_exr_slots(d_in_len, d_images, d_channels, chan_cap, n_files, d_sel, n_sel, 1u, chunk_cap, decoded_bytes, d_pcap, d_ch_off, d_raw_off,
                             d_size, d_nch, d_rawb, d_kind, d_live, stream);
        if (chunk_cap) {
            zmi_launch_exr_chunks(in, d_in_off, d_in_len, d_images, d_channels, chan_cap, d_sel, n_sel, d_ch_off, d_live, chunk_cap, d_zin_off, d_zin_len,
                                  d_csz, d_rawlen, d_fl, d_items, d_nblk, d_cslot, d_cm, d_pitems, stream);
            zmi_launch_scan_sizes(d_items, chunk_cap, d_item_off, stream);
            zmi_launch_scan_sizes(d_pitems, chunk_cap, d_pitem_off, stream);
            zmi_launch_scan_sizes(d_nblk, chunk_cap, d_blk_off, stream);
        }
    }
    if (chunk_cap) {
        rc = zmi_inflate_packed_body(c, d_in, d_zin_off, d_zin_len, chunk_cap, ZMI_WRAP_ZLIB, nullptr, 0u, d_csz, d_scap, 16u, d_sbuf, scan_cap, d_soff,
                                     d_slen, d_sst, d_sused, d_sdet, ZMI_K_PARSE, stream_, d_cm, d_dcap);
        if (rc) return rc;
        {
            // chunks stored raw: their bytes as they stand (max_len only shapes the launch)
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_copy_ranges(in, d_zin_off, 0u, d_rawlen, chunk_cap, d_sbuf, d_soff, scan_cap,
                                   decoded_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)decoded_bytes, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_ENCODE, stream);
            zmi_launch_exr_blocksum(d_sbuf, d_soff, d_csz, d_scap, d_blk_off, chunk_cap, nblk, d_bsum, d_bpre, stream);
            zmi_launch_exr_unzip(d_images, d_channels, chan_cap, d_sel, d_ch_off, d_cslot, chunk_cap, d_item_off, decoded_bytes / 2u, d_sbuf,
                                 d_soff, d_csz, d_scap, d_slen, d_sst, d_rawlen, d_blk_off, d_bpre, (uint8_t*)d_out, d_out_off, stream);
            zmi_launch_exr_pxr24_undo(d_images, d_channels, chan_cap, d_sel, d_ch_off, d_cslot, chunk_cap, d_pitem_off, decoded_bytes / 2u, d_sbuf,
                                      d_soff, d_csz, d_scap, d_cm, d_slen, d_sst, (uint8_t*)d_out, d_out_off, stream);
        }
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_exr_finish(d_images, d_sel, n_sel, d_kind, d_size, d_pcap, d_ch_off, d_raw_off, chunk_cap, decoded_bytes, d_csz, d_scap, d_rawlen,
                              d_fl, d_cm, d_slen, d_sst, d_out_len, d_status, d_detail, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- writing PNG images (include/zmi355.h; the kernels: png_kernels.h, checksum.hip) -------------------------------
// zmi_zip_write_dev's plan with the filtered scanlines in place of the entries: the filter kernel writes every image's scanlines into
// context scratch, their pieces are one table of at most n_images + scan_bytes / piece_bytes places that goes through the
// independent-piece encoder in launch groups (chain mode 2 with the bitmap of the pieces that end an image's stream); a group's payloads
// are checksummed where they stand in the slots and placed behind the device word the group before ended at; the 43 + 20 fixed bytes
// around every image's payload are written once the last group is in place.
extern "C" uint64_t zmi_png_bound(uint32_t n_images, uint64_t scan_bytes, uint32_t piece_bytes, uint32_t out_align, int level) {
    (void)level;
    if (piece_bytes == 0) return 0;
    // signature, IHDR, IDAT frame, zlib frame and IEND, and the pad, per image; per piece the slot of zmi_deflate_pieces_stride and the
    // block headers of its regions
    return (uint64_t)n_images * (63u + (uint64_t)(out_align ? out_align - 1u : 0u)) + scan_bytes + (scan_bytes >> 3) +
           ((uint64_t)n_images + scan_bytes / piece_bytes) * 160u;
}

extern "C" int zmi_png_encode_dev(zmi_ctx* c, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_png_image* d_images,
                                  uint32_t n, uint64_t scan_bytes, uint32_t flags, uint32_t filter, uint32_t piece_bytes, int level, int strategy,
                                  uint32_t out_align, void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len,
                                  zmi_png_image* d_written, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    int rc = zmi_check_piece_bytes(piece_bytes);
    if (!rc) rc = zmi_check_level_strategy(level, strategy);
    if (!rc) rc = zmi_check_out_align(out_align);
    if (rc) return rc;
    if (flags & ~ZMI_PNG_NATIVE16) return zmi_fail(ZMI_E_ARG, "unknown flag");
    if (filter > ZMI_PNG_FILTER_ADAPTIVE) return zmi_fail(ZMI_E_ARG, "filter must be 0 .. 4 or ZMI_PNG_FILTER_ADAPTIVE");
    if (n > 0x7FFFFFFFu) return zmi_fail(ZMI_E_ARG, "zmi_png_encode_dev: more than 2^31 - 1 images");
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    if ((out_cap && !d_out) || (n && (!d_in_off || !d_in_len || !d_images || !d_out_len || !d_status || (scan_bytes && !d_in))))
        return zmi_fail(ZMI_E_ARG, "null argument");
    const uint64_t np64 = n ? (uint64_t)n + scan_bytes / piece_bytes : 0u;
    if (np64 > 0x7FFFFFFFull) return zmi_fail(ZMI_E_ARG, "zmi_png_encode_dev: more than 2^31 - 1 pieces");
    if (scan_bytes > (1ull << 44)) return zmi_fail(ZMI_E_NOMEM, "scan_bytes sizes the scratch: give the bound there is");
    const uint32_t np = (uint32_t)np64;
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    if (n == 0) {
        ZMI_HIP(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), stream));
        return ZMI_E_OK;
    }

    // launch groups and slots: zmi_zip_write_dev's, at every level (level 0 is deflate stored blocks from the same encoder)
    const uint32_t max_len = scan_bytes < piece_bytes ? (uint32_t)scan_bytes : piece_bytes;
    const uint64_t stride = zmi_piece_slot_stride(max_len, piece_bytes, level);
    zmi_group_plan plan;
    rc = zmi_plan_slots(c, np, max_len, stride, "scratch limit too small for one piece", &plan);
    if (rc) return rc;
    const uint64_t group = plan.group;
    const uint32_t wpg = plan.wpg;
    const size_t bm_words = plan.bm_words;

    uint64_t *d_first, *d_soff, *d_item_off, *d_poff, *d_pos, *d_slot_off;
    zmi_words4 neff;
    uint32_t *d_ssz, *d_nlen, *d_npc, *d_bands, *d_iadler, *d_icrc, *d_plen, *d_head, *d_olen, *d_padler, *d_pcrc, *d_slot_len, *d_ends;
    int32_t* d_st;
    uint8_t* d_scan;
    rc = zmi_carve(c->png, [&](zmi_carver k) {
        k.take(n + 1u, d_first, d_soff, d_item_off);                     // per image: its first piece, scanline offset, first band
        k.take(np, d_poff);                                              // per piece: its place in the scanlines
        k.take(np + 1u, d_pos);                                          // ... and in d_out
        k.take(group, d_slot_off);                                       // the slots of a group
        k.take(neff);                                                    // the count that is valid; the sum of the scanline sizes (u64)
        k.take(n, d_ssz, d_nlen, d_npc, d_bands, d_iadler, d_icrc);      // per image: scanline size, hole, pieces, bands, Adler-32, CRC-32
        k.take(np, d_plen, d_head, d_olen, d_st, d_padler, d_pcrc);      // per piece: length, hole, encoder's size and status, Adler-32, CRC-32
        k.take(group, d_slot_len);                                       // a table the slot layout fills
        k.take(bm_words, d_ends);                                        // the bitmap of the pieces that end an image's stream
        k.skip(16u);                                                     // (spare: the reservation has always had it)
        k.align(256u);
        k.region(d_scan, scan_bytes, 64u);                               // the filtered scanlines
        return k.end();
    });
    if (rc) return rc;
    uint32_t* const d_neff = neff.w;
    uint64_t* const d_sum = neff.upper64();             // (zmi_png_wlayout_kernel)
    int32_t* const d_call = (int32_t*)neff.word(1);     // (the slots carry the pieces kernel's status here)

    ZMI_HIP(hipMemsetAsync(d_pos, 0, 8, stream));     // where the first group's pack starts
    ZMI_HIP(hipMemsetAsync(d_neff, 0, 16, stream));
    ZMI_HIP(hipMemsetAsync(d_ends, 0, bm_words * 4u, stream));
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_png_wlayout(d_images, d_in_len, n, piece_bytes, d_ssz, d_nlen, d_npc, d_bands, d_sum, stream);
        zmi_launch_scan_sizes(d_npc, n, d_first, stream);
        zmi_launch_scan_sizes(d_ssz, n, d_soff, stream);
        zmi_launch_scan_sizes(d_bands, n, d_item_off, stream);
        zmi_launch_zip_pieces(d_soff, d_ssz, d_nlen, d_first, d_sum, n, scan_bytes, piece_bytes, np, (uint32_t)group, wpg, d_poff, d_plen, d_head,
                              d_ends, d_neff, d_call, stream);
        zmi_launch_piece_layout(group * stride, (uint32_t)stride, (uint32_t)group, d_slot_off, d_slot_len, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_INFLATE, stream);
        zmi_launch_png_filter(d_images, (const uint8_t*)d_in, d_in_off, d_in_len, n, d_item_off, d_sum, scan_bytes, d_scan, d_soff, filter,
                              (flags & ZMI_PNG_NATIVE16) ? 1u : 0u, stream);
    }
    rc = zmi_piece_checks(c, d_scan, d_poff, d_plen, np, ZMI_WRAP_ZLIB, d_padler, stream);
    if (rc) return rc;
    for (uint64_t first = 0; first < np; first += group) {
        const uint32_t cnt = (uint32_t)(np - first < group ? np - first : group);
        const uint32_t* d_gends = d_ends + (first / group) * wpg;
        rc = zmi_deflate_impl(c, {.d_in = d_scan, .d_in_off = d_poff + first, .d_in_len = d_plen + first, .n = cnt, .max_len = max_len,
                                  .level = level, .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = 2u, .d_out = c->sd_slots.p,
                                  .out_stride = stride, .d_out_len = d_olen + first, .d_status = d_st + first, .stream = stream_, .carry = 0,
                                  .ends = d_gends, .geom_len = piece_bytes});
        if (rc) return rc;
        {
            // the IDAT CRC-32 covers the COMPRESSED bytes: every piece's where it stands in its slot, folded per image below
            zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
            zmi_launch_checksum((const uint8_t*)c->sd_slots.p, d_slot_off, d_olen + first, cnt, 2u, d_pcrc + first, d_pcrc + first, stream);
        }
        // the group's pieces go behind the previous group's, the running offset never leaves the device
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_png_place(d_head + first, d_olen + first, d_gends, cnt, out_align, d_pos + first, stream);
        zmi_launch_zip_pack(nullptr, d_poff + first, d_head + first, (const uint8_t*)c->sd_slots.p, stride, d_olen + first, cnt,
                            stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride, (uint8_t*)d_out, d_pos + first, out_cap, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_combine_segments_adler(d_padler, d_plen, d_first, n, d_neff, d_iadler, stream);
        zmi_launch_combine_segments(d_pcrc, d_olen, d_first, n, d_neff, d_icrc, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_png_wfinish(d_images, d_in_len, n, d_neff, d_first, d_pos, d_olen, d_st, d_iadler, d_icrc, (uint32_t)level, (uint32_t)strategy,
                               (uint8_t*)d_out, out_cap, d_out_off, d_out_len, d_status, d_written, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- writing TIFF files (include/zmi355.h; the kernels: tiff_write_kernels.h, checksum.hip) -------------------------
// zmi_png_encode_dev's plan with the predicted segments in place of the filtered scanlines.  The geometry is host data, so the plan,
// the metadata's bytes and the record of the written page are made here (zmi_tiff_wplan) and handed to the kernels by value.
static void zmi_tw_le(uint8_t* p, uint64_t v, uint32_t nb) { for (uint32_t i = 0; i < nb; ++i) p[i] = (uint8_t)(v >> (8u * i)); }
// NULL, or what is wrong with *w
static const char* zmi_tiff_wplan(const zmi_tiff_write* w, int* level_out, zmi_tw_plan* g, zmi_tw_meta* m) {
    if (!w) return "zmi_tiff_write: null";
    if (w->width == 0u || w->height == 0u) return "zmi_tiff_write: a dimension of 0";
    if (w->bits != 8u && w->bits != 16u && w->bits != 32u && w->bits != 64u) return "zmi_tiff_write: bits must be 8, 16, 32 or 64";
    if (w->samples == 0u || w->samples > 8u) return "zmi_tiff_write: samples must be 1 .. 8";
    if (w->extra_samples >= w->samples) return "zmi_tiff_write: extra_samples must be below samples";
    if (w->predictor < 1u || w->predictor > 3u) return "zmi_tiff_write: predictor must be 1 .. 3";
    if (w->sample_format < 1u || w->sample_format > 3u) return "zmi_tiff_write: sample_format must be 1 .. 3";
    if (w->predictor == 3u && (w->sample_format != 3u || w->bits < 16u)) return "zmi_tiff_write: predictor 3 needs sample_format 3 and bits >= 16";
    if ((w->tile_w == 0u) != (w->tile_h == 0u)) return "zmi_tiff_write: tile_w and tile_h must both be 0 or both be set";
    if (w->tile_w % 16u != 0u || w->tile_h % 16u != 0u) return "zmi_tiff_write: a tile size must be a multiple of 16";
    const bool tiled = w->tile_w != 0u;
    const uint32_t sb = w->bits / 8u, pb = sb * w->samples;
    const uint32_t seg_w = tiled ? w->tile_w : w->width;
    const uint32_t seg_h = tiled ? w->tile_h : (w->rows_per_strip == 0u || w->rows_per_strip >= w->height ? w->height : w->rows_per_strip);
    const uint64_t rb = (uint64_t)seg_w * pb, seg_bytes = rb * seg_h;
    if (seg_bytes > ZMI_PNG_SCAN_MAX) return "zmi_tiff_write: a segment's decoded size passes ZMI_PNG_SCAN_MAX";
    if (w->piece_bytes == 0u || w->piece_bytes > (1u << 30)) return "zmi_tiff_write: piece_bytes must be 1 .. 2^30";
    int level = w->level;
    if (level == -1) level = 6;
    if (level < 0 || level > 9) return "zmi_tiff_write: level must be -1 .. 9";
    if (w->strategy < 0 || w->strategy > 4) return "zmi_tiff_write: strategy must be 0 .. 4";
    if (w->out_align == 0u || w->out_align > 4096u || (w->out_align & (w->out_align - 1u)) != 0u)
        return "zmi_tiff_write: out_align must be a power of two, 1 .. 4096";
    if (w->flags & ~(ZMI_TIFF_ASSEMBLE | ZMI_TIFF_BIGTIFF)) return "zmi_tiff_write: unknown flag";
    const uint64_t across = ((uint64_t)w->width + seg_w - 1u) / seg_w, down = ((uint64_t)w->height + seg_h - 1u) / seg_h;
    const uint64_t n_segs = across * down;
    const uint32_t last_rows = tiled ? seg_h : (uint32_t)(w->height - (down - 1u) * seg_h);
    const uint64_t last_bytes = rb * last_rows;
    if (n_segs > 0x7FFFFFFFull) return "zmi_tiff_write: more than 2^31 - 1 pieces";
    const uint64_t scan = (n_segs - 1u) * seg_bytes + last_bytes;
    if (n_segs + scan / w->piece_bytes > 0x7FFFFFFFull) return "zmi_tiff_write: more than 2^31 - 1 pieces";
    const bool big = (w->flags & ZMI_TIFF_BIGTIFF) != 0u;
    *level_out = level;
    memset(g, 0, sizeof *g);
    memset(m, 0, sizeof *m);
    g->width = w->width; g->height = w->height; g->seg_w = seg_w; g->seg_h = seg_h; g->across = (uint32_t)across; g->n_segs = (uint32_t)n_segs;
    g->sb = sb; g->spp = w->samples; g->pb = pb; g->rb = (uint32_t)rb;
    g->pred = w->predictor; g->assemble = (w->flags & ZMI_TIFF_ASSEMBLE) ? 1u : 0u; g->big = big ? 1u : 0u;
    g->seg_bytes = (uint32_t)seg_bytes; g->last_bytes = (uint32_t)last_bytes;
    g->ss = (uint32_t)((seg_bytes + 15u) & ~15ull);
    g->piece_bytes = w->piece_bytes;
    g->ppf = (uint32_t)((seg_bytes + w->piece_bytes - 1u) / w->piece_bytes);
    g->ppl = (uint32_t)((last_bytes + w->piece_bytes - 1u) / w->piece_bytes);
    g->np = (uint32_t)((n_segs - 1u) * g->ppf + g->ppl);
    // a band of rows, the predict kernel's work item: about 8 KiB of a segment, one row at least, 8 at most
    g->band_rows = rb >= 8192u ? 1u : (8192u / (uint32_t)rb > 8u ? 8u : 8192u / (uint32_t)rb);
    g->bands = (seg_h + g->band_rows - 1u) / g->band_rows;

    // the entries, ascending by tag: {tag, type (3 SHORT, 4 LONG, 16 LONG8), count, the value repeated `count` times}; the two arrays are
    // written by the segments' kernel where `arr` says so
    struct ent { uint32_t tag, type; uint64_t count, value; bool arr; };
    const uint32_t seg_t = big ? 16u : 4u;
    ent e[14];
    uint32_t ne = 0;
    e[ne++] = {256u, 4u, 1u, w->width, false};
    e[ne++] = {257u, 4u, 1u, w->height, false};
    e[ne++] = {258u, 3u, w->samples, w->bits, false};
    e[ne++] = {259u, 3u, 1u, 8u, false};
    e[ne++] = {262u, 3u, 1u, w->photometric, false};
    if (!tiled) e[ne++] = {273u, seg_t, n_segs, 0u, true};
    e[ne++] = {277u, 3u, 1u, w->samples, false};
    if (!tiled) {
        e[ne++] = {278u, 4u, 1u, seg_h, false};
        e[ne++] = {279u, seg_t, n_segs, 0u, true};
    }
    e[ne++] = {284u, 3u, 1u, 1u, false};
    e[ne++] = {317u, 3u, 1u, w->predictor, false};
    if (tiled) {
        e[ne++] = {322u, 4u, 1u, seg_w, false};
        e[ne++] = {323u, 4u, 1u, seg_h, false};
        e[ne++] = {324u, seg_t, n_segs, 0u, true};
        e[ne++] = {325u, seg_t, n_segs, 0u, true};
    }
    if (w->extra_samples) e[ne++] = {338u, 3u, w->extra_samples, w->extra_kind, false};
    e[ne++] = {339u, 3u, w->samples, w->sample_format, false};
    const uint32_t os = big ? 8u : 4u, es = big ? 20u : 12u, cs = big ? 8u : 2u, ifd = big ? 16u : 8u;
    uint8_t* b = m->b;
    b[0] = b[1] = 0x49u; b[2] = big ? 0x2Bu : 0x2Au; b[4] = 8u;
    if (big) zmi_tw_le(b + 8, 16u, 8u);
    zmi_tw_le(b + ifd, ne, cs);
    uint64_t at = ifd + cs + (uint64_t)ne * es + os;     // where the next out-of-line value goes (always even: every value is 2, 4 or 8 bytes)
    m->a_len = (uint32_t)at;
    bool behind = false;                                 // behind the two arrays: part b of the metadata
    uint64_t arr_pos[2] = {0u, 0u};
    uint32_t n_arr = 0;
    for (uint32_t q = 0; q < ne; ++q) {
        uint8_t* f = b + ifd + cs + (size_t)q * es;
        const uint32_t ts = e[q].type == 3u ? 2u : (e[q].type == 4u ? 4u : 8u);
        const uint64_t bytes = e[q].count * ts;
        zmi_tw_le(f, e[q].tag, 2u);
        zmi_tw_le(f + 2, e[q].type, 2u);
        zmi_tw_le(f + 4, e[q].count, os);
        uint64_t vpos = ifd + cs + (uint64_t)q * es + 4u + os;   // inline
        if (bytes > os) {
            vpos = at;
            zmi_tw_le(f + 4 + os, at, os);
            at += bytes;
        }
        if (e[q].arr) {
            arr_pos[n_arr++] = vpos;
            if (bytes > os) { behind = true; m->b_pos = at; }
            continue;
        }
        uint8_t* v;
        if (bytes <= os) v = f + 4 + os;
        else if (!behind) { v = b + vpos; m->a_len = (uint32_t)at; }
        else { v = b + m->a_len + (vpos - m->b_pos); m->b_len = (uint32_t)(at - m->b_pos); }
        for (uint64_t i = 0; i < e[q].count; ++i) zmi_tw_le(v + i * ts, e[q].value, ts);
    }
    g->off_pos = arr_pos[0]; g->cnt_pos = arr_pos[1];
    g->meta_end = at;
    g->seg0 = (at + w->out_align - 1u) & ~(uint64_t)(w->out_align - 1u);

    zmi_tiff_page r;
    memset(&r, 0, sizeof r);
    r.offsets_pos = arr_pos[0]; r.counts_pos = arr_pos[1];
    r.width = w->width; r.height = w->height; r.seg_w = seg_w; r.seg_h = seg_h;
    r.segs_across = (uint32_t)across; r.segs_down = (uint32_t)down; r.n_segs = (uint32_t)n_segs; r.seg_bytes = (uint32_t)seg_bytes;
    r.bits = w->bits; r.samples = w->samples; r.sample_format = w->sample_format; r.predictor = w->predictor; r.compression = 8u;
    r.photometric = w->photometric; r.extra_samples = w->extra_samples;
    r.sample_bytes = (uint8_t)sb; r.big_endian = 0u; r.bigtiff = big ? 1u : 0u; r.tiled = tiled ? 1u : 0u;
    r.offsets_type = r.counts_type = (uint8_t)seg_t;
    static_assert(sizeof r == sizeof m->rec, "zmi_tiff_page is 72 bytes");
    memcpy(m->rec, &r, sizeof r);
    return nullptr;
}

extern "C" uint64_t zmi_tiff_bound(const zmi_tiff_write* w) {
    zmi_tw_plan g;
    zmi_tw_meta m;
    int level;
    if (zmi_tiff_wplan(w, &level, &g, &m)) return 0;
    // the metadata and its pad; the zlib frame and the pad per segment; per piece the slot of zmi_deflate_pieces_stride and the block
    // headers of its regions, as zmi_png_bound
    const uint64_t scan = (uint64_t)(g.n_segs - 1u) * g.seg_bytes + g.last_bytes;
    return g.seg0 + (uint64_t)g.n_segs * (6u + (uint64_t)(w->out_align - 1u)) + scan + (scan >> 3) + (uint64_t)g.np * 160u;
}

extern "C" int zmi_tiff_write_dev(zmi_ctx* c, const zmi_tiff_write* w, const void* d_in, const uint64_t* d_in_off, void* d_out, uint64_t out_cap,
                                  uint64_t* d_file_len, uint32_t* d_seg_len, int32_t* d_status, int32_t* d_file_status, zmi_tiff_page* d_written,
                                  void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    zmi_tw_plan g;
    zmi_tw_meta meta;
    int level = 0;
    if (const char* what = zmi_tiff_wplan(w, &level, &g, &meta)) return zmi_fail(ZMI_E_ARG, what);
    if (!d_in || (!g.assemble && !d_in_off) || (out_cap && !d_out) || !d_file_len || !d_status || !d_file_status)
        return zmi_fail(ZMI_E_ARG, "null argument");
    const int strategy = w->strategy;
    const uint32_t piece_bytes = w->piece_bytes, n = g.n_segs, np = g.np;
    if ((uint64_t)n * g.ss > (1ull << 44)) return zmi_fail(ZMI_E_NOMEM, "the page's decoded bytes size the scratch");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);

    // launch groups and slots: zmi_png_encode_dev's, but the host knows the longest piece there is -- a full segment, or piece_bytes
    // where that is less -- so slots and match scratch follow the segments (a 192 KiB tile under piece_bytes of 1 MiB takes a fifth of
    // what a 1 MiB piece would) while geom_len = piece_bytes keeps the bytes those of pieces of piece_bytes
    const uint32_t max_len = g.seg_bytes < piece_bytes ? g.seg_bytes : piece_bytes;
    const uint64_t stride = zmi_piece_slot_stride(max_len, piece_bytes, level);
    zmi_group_plan plan;
    int rc = zmi_plan_slots(c, np, max_len, stride, "scratch limit too small for one piece", &plan);
    if (rc) return rc;
    const uint64_t group = plan.group;
    const uint32_t wpg = plan.wpg;
    const size_t bm_words = plan.bm_words;

    uint64_t *d_first, *d_poff, *d_pos, *d_slot_off;
    zmi_words4 neff;
    uint32_t *d_sadler, *d_plen, *d_head, *d_olen, *d_padler, *d_slot_len, *d_ends;
    int32_t* d_st;
    uint8_t* d_scan;
    rc = zmi_carve(c->tiff_w, [&](zmi_carver k) {
        k.take(n + 1u, d_first);         // per segment: its first piece
        k.take(np, d_poff);              // per piece: its place in the scratch
        k.take(np + 1u, d_pos);          // ... in d_out
        k.take(group, d_slot_off);       // the slots of a group
        k.take(neff);                    // the segments that are live: all | the first segment with a status
        k.take(n, d_sadler);             // per segment: the Adler-32
        k.take(np, d_plen, d_head, d_olen, d_st, d_padler);   // per piece: length, hole, encoder's size and status, Adler-32
        k.take(group, d_slot_len);       // a table the slot layout fills
        k.take(bm_words, d_ends);        // the bitmap of the pieces that end a segment's stream
        k.skip(16u);                     // (spare: the reservation has always had it)
        k.align(256u);
        k.region(d_scan, (size_t)n * g.ss, 64u);   // the predicted segments, every one at a multiple of 16
        return k.end();
    });
    if (rc) return rc;
    uint32_t* const d_neff = neff.w;
    uint32_t* const d_bad = neff.word(1);

    ZMI_HIP(hipMemsetAsync(d_bad, 0xFF, 4, stream));
    ZMI_HIP(hipMemsetAsync(d_ends, 0, bm_words * 4u, stream));
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_tiff_wpieces(g, (uint32_t)group, wpg, d_poff, d_plen, d_head, d_ends, d_first, d_neff, d_pos, stream);
        zmi_launch_piece_layout(group * stride, (uint32_t)stride, (uint32_t)group, d_slot_off, d_slot_len, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_INFLATE, stream);
        zmi_launch_tiff_predict(g, (const uint8_t*)d_in, d_in_off, d_scan, stream);
    }
    rc = zmi_piece_checks(c, d_scan, d_poff, d_plen, np, ZMI_WRAP_ZLIB, d_padler, stream);
    if (rc) return rc;
    for (uint64_t first = 0; first < np; first += group) {
        const uint32_t cnt = (uint32_t)(np - first < group ? np - first : group);
        const uint32_t* d_gends = d_ends + (first / group) * wpg;
        rc = zmi_deflate_impl(c, {.d_in = d_scan, .d_in_off = d_poff + first, .d_in_len = d_plen + first, .n = cnt, .max_len = max_len,
                                  .level = level, .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = 2u, .d_out = c->sd_slots.p,
                                  .out_stride = stride, .d_out_len = d_olen + first, .d_status = d_st + first, .stream = stream_, .carry = 0,
                                  .ends = d_gends, .geom_len = piece_bytes});
        if (rc) return rc;
        // the group's pieces go behind the previous group's, the running offset never leaves the device
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_tiff_place(d_head + first, d_olen + first, d_gends, cnt, w->out_align, d_pos + first, stream);
        zmi_launch_zip_pack(nullptr, d_poff + first, d_head + first, (const uint8_t*)c->sd_slots.p, stride, d_olen + first, cnt,
                            stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride, (uint8_t*)d_out, d_pos + first, out_cap, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_combine_segments_adler(d_padler, d_plen, d_first, n, d_neff, d_sadler, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_tiff_wmeta(meta, (uint8_t*)d_out, out_cap, stream);
        zmi_launch_tiff_wsegs(g, d_pos, d_olen, d_st, d_sadler, (uint32_t)level, (uint32_t)strategy, (uint8_t*)d_out, out_cap, d_seg_len, d_status,
                              d_bad, stream);
        zmi_launch_tiff_wclose(g, meta, d_pos, d_olen, d_status, d_bad, out_cap, d_file_len, d_file_status, d_written, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- writing OpenEXR images (include/zmi355.h; the kernels: exr_write_kernels.h, checksum.hip) ----------------------
// zmi_tiff_write_dev's plan with chunks in place of segments and one more step: the place kernel of a launch group decides per chunk
// between the candidate stream and the raw bytes, so a group holds whole chunks.  The layout is host data: the plan, the header's bytes
// and the records of a written file are made here (zmi_exr_wplan); the plan goes to the kernels by value, the channel records and the
// header's bytes through kernel arguments into the scratch (they have no fixed size).
struct zmi_xw_host {
    zmi_xw_plan g;
    std::vector<uint8_t> blob;       // n_ch zmi_exr_channel records | the header's hdr_len bytes
    uint64_t file_bound = 0;         // header + table + every chunk's header + n
    uint64_t ppi = 0, ssi = 0, ipi = 0;   // per image: pieces, bytes of d in the scratch, work items of the forward kernel
    uint64_t fpi = 0;                // ... the trips of the PXR24 forward (compression 5)
    uint32_t n_max = 0;              // the bytes of d of the largest chunk: its raw size, m under PXR24
    uint64_t pp[2][2] = {{0, 0}, {0, 0}};   // the pieces of a chunk in an inner / the last column [0 / 1], an inner / the last row
};
static void zmi_xw_attr(std::vector<uint8_t>& b, const char* name, const char* type, const void* value, uint32_t size) {
    b.insert(b.end(), (const uint8_t*)name, (const uint8_t*)name + strlen(name) + 1u);
    b.insert(b.end(), (const uint8_t*)type, (const uint8_t*)type + strlen(type) + 1u);
    uint8_t s[4];
    zmi_tw_le(s, size, 4u);
    b.insert(b.end(), s, s + 4);
    b.insert(b.end(), (const uint8_t*)value, (const uint8_t*)value + size);
}
// the checks every container writer shares (their texts stand once, above); *level: -1 resolved
static int zmi_exr_wcheck(const zmi_exr_write* w, int* level) {
    if (!w) return zmi_fail(ZMI_E_ARG, "zmi_exr_write: null");
    *level = w->level;
    int rc = zmi_check_piece_bytes(w->piece_bytes);
    if (!rc) rc = zmi_check_level_strategy(*level, w->strategy);
    if (!rc) rc = zmi_check_out_align(w->out_align);
    return rc;
}
// NULL, or what else is wrong with *w (zmi_exr_wcheck has passed)
static const char* zmi_exr_wplan(const zmi_exr_write* w, uint32_t n_images, zmi_xw_host* h) {
    if (w->data_window[2] < w->data_window[0] || w->data_window[3] < w->data_window[1]) return "zmi_exr_write: an inverted data window";
    if (w->display_window[2] < w->display_window[0] || w->display_window[3] < w->display_window[1]) return "zmi_exr_write: an inverted display window";
    if (w->n_channels == 0u || !w->channels) return "zmi_exr_write: no channels";
    if (w->compression != 0u && w->compression != 2u && w->compression != 3u && w->compression != 5u)
        return "zmi_exr_write: compression must be 0 (NONE), 2 (ZIPS), 3 (ZIP) or 5 (PXR24)";
    if ((w->tile_w == 0u) != (w->tile_h == 0u)) return "zmi_exr_write: tile_w and tile_h must both be 0 or both be set";
    if (w->flags != 0u) return "zmi_exr_write: unknown flag";
    bool long_names = false;
    uint64_t per_px = 0, per_p = 0;
    for (uint32_t c = 0; c < w->n_channels; ++c) {
        const zmi_exr_write_channel& ch = w->channels[c];
        if (ch.pixel_type < 0 || ch.pixel_type > 2) return "zmi_exr_write: a pixel type must be 0 (UINT), 1 (HALF) or 2 (FLOAT)";
        if (!ch.name || ch.name[0] == 0) return "zmi_exr_write: an empty channel name";
        const size_t nl = strnlen(ch.name, 256u);
        if (nl > 255u) return "zmi_exr_write: a channel name longer than 255 bytes";
        if (nl > 31u) long_names = true;
        if (c && strcmp(w->channels[c - 1u].name, ch.name) >= 0) return "zmi_exr_write: channel names must be strictly ascending";
        per_px += ch.pixel_type == 1 ? 2u : 4u;
        per_p += ch.pixel_type == 1 ? 2u : (ch.pixel_type == 2 ? 3u : 4u);
    }
    // what xr_geometry (exr_kernels.h) calls big
    const uint64_t W = (uint64_t)((int64_t)w->data_window[2] - (int64_t)w->data_window[0] + 1);
    const uint64_t H = (uint64_t)((int64_t)w->data_window[3] - (int64_t)w->data_window[1] + 1);
    const char* big = "zmi_exr_write: the image does not fit 32 bits (width, height, pixels, a row, the region or a chunk)";
    if (W > 0xFFFFFFFFull || H > 0xFFFFFFFFull || W * H > 0xFFFFFFFFull || per_px > 0xFFFFFFFFull) return big;
    const bool tiled = w->tile_w != 0u;
    const bool pxr24 = w->compression == 5u;
    const uint32_t lines = w->compression == 3u || pxr24 ? 16u : 1u;
    const uint64_t box_w = tiled ? w->tile_w : W, box_h = tiled ? w->tile_h : lines;
    const uint64_t cw0 = box_w < W ? box_w : W, rows0 = box_h < H ? box_h : H;
    uint64_t region = 0;
    for (uint32_t c = 0; c < w->n_channels; ++c) region = ((region + 3u) & ~3ull) + W * H * (w->channels[c].pixel_type == 1 ? 2u : 4u);
    if (W * per_px > 0xFFFFFFFFull || region > 0xFFFFFFFFull || rows0 * cw0 * per_px > 0xFFFFFFFFull) return big;
    const uint64_t across = (W + box_w - 1u) / box_w, down = (H + box_h - 1u) / box_h;
    if (across > 0x7FFFFFFFull / down || across * down * (n_images ? n_images : 1u) > 0x7FFFFFFFull)
        return "zmi_exr_write: more than 2^31 - 1 chunks";
    const uint64_t nc = across * down;
    const bool none = w->compression == 0u;

    // the header
    std::vector<uint8_t> hd = {0x76u, 0x2Fu, 0x31u, 0x01u, 0u, 0u, 0u, 0u};
    zmi_tw_le(hd.data() + 4, 2u | (tiled ? 0x200u : 0u) | (long_names ? 0x400u : 0u), 4u);
    std::vector<uint8_t> chl;
    std::vector<uint32_t> name_pos(w->n_channels);
    const uint32_t chl_at = 8u + 9u + 7u + 4u;                             // "channels\0" "chlist\0" size
    for (uint32_t c = 0; c < w->n_channels; ++c) {
        const char* nm = w->channels[c].name;
        name_pos[c] = chl_at + (uint32_t)chl.size();
        chl.insert(chl.end(), (const uint8_t*)nm, (const uint8_t*)nm + strlen(nm) + 1u);
        uint8_t e[16] = {0};
        zmi_tw_le(e, (uint32_t)w->channels[c].pixel_type, 4u);
        zmi_tw_le(e + 8, 1u, 4u);
        zmi_tw_le(e + 12, 1u, 4u);
        chl.insert(chl.end(), e, e + 16);
    }
    chl.push_back(0u);
    if (chl.size() > 0x7FFFFFFFull) return "zmi_exr_write: the channel list passes 2^31 - 1 bytes";
    uint8_t box[16], one[4], zero8[8] = {0}, v1[1], td[9];
    zmi_tw_le(one, 0x3F800000u, 4u);
    zmi_xw_attr(hd, "channels", "chlist", chl.data(), (uint32_t)chl.size());
    v1[0] = (uint8_t)w->compression;
    zmi_xw_attr(hd, "compression", "compression", v1, 1u);
    for (uint32_t k = 0; k < 4u; ++k) zmi_tw_le(box + 4u * k, (uint32_t)w->data_window[k], 4u);
    zmi_xw_attr(hd, "dataWindow", "box2i", box, 16u);
    for (uint32_t k = 0; k < 4u; ++k) zmi_tw_le(box + 4u * k, (uint32_t)w->display_window[k], 4u);
    zmi_xw_attr(hd, "displayWindow", "box2i", box, 16u);
    v1[0] = 0u;
    zmi_xw_attr(hd, "lineOrder", "lineOrder", v1, 1u);
    zmi_xw_attr(hd, "pixelAspectRatio", "float", one, 4u);
    zmi_xw_attr(hd, "screenWindowCenter", "v2f", zero8, 8u);
    zmi_xw_attr(hd, "screenWindowWidth", "float", one, 4u);
    if (tiled) {
        zmi_tw_le(td, w->tile_w, 4u);
        zmi_tw_le(td + 4, w->tile_h, 4u);
        td[8] = 0u;
        zmi_xw_attr(hd, "tiles", "tiledesc", td, 9u);
    }
    hd.push_back(0u);
    const uint64_t hdr_len = hd.size();
    const uint32_t chdr = tiled ? 20u : 8u;
    const uint64_t file_bound = hdr_len + nc * (8u + chdr) + H * W * per_px;
    if (file_bound > 0xFFFFFFFFull) return "zmi_exr_write: a file may pass 2^32 - 1 bytes";

    // the four sizes a chunk has: inner or last column, inner or last row
    const uint64_t cw_last = W - (across - 1u) * box_w, rows_last = H - (down - 1u) * box_h;
    uint64_t ppi = 0, ssi = 0, ipi = 0, fpi = 0;
    for (uint32_t cx = 0; cx < 2u; ++cx)
        for (uint32_t cy = 0; cy < 2u; ++cy) {
            const uint64_t count = (cx ? 1u : across - 1u) * (cy ? 1u : down - 1u);
            const uint64_t cw = cx ? cw_last : cw0, rows = cy ? rows_last : rows0, n = rows * cw * per_px;
            uint64_t per_row = 0;
            for (uint32_t c = 0; c < w->n_channels; ++c) per_row += (cw * (w->channels[c].pixel_type == 1 ? 2u : 4u) + 8191u) / 8192u;   // (XW_PIECE)
            ipi += count * rows * per_row;
            if (pxr24) fpi += count * rows * w->n_channels * ((cw + 255u) / 256u);                                                      // (XW_P24_TRIP)
            if (!none) {
                const uint64_t m = pxr24 ? rows * cw * per_p : n;          // the bytes of the chunk's d
                h->pp[cx][cy] = (m + w->piece_bytes - 1u) / w->piece_bytes;
                ppi += count * h->pp[cx][cy];
                ssi += count * ((m + 15u) & ~15ull);
            }
        }
    if (ppi * (n_images ? n_images : 1u) > 0x7FFFFFFFull) return "zmi_exr_write: more than 2^31 - 1 pieces";

    zmi_xw_plan& g = h->g;
    memset(&g, 0, sizeof g);
    g.W = (uint32_t)W; g.H = (uint32_t)H; g.box_w = (uint32_t)(box_w > 0xFFFFFFFFull ? 0xFFFFFFFFull : box_w); g.box_h = (uint32_t)box_h;
    g.across = (uint32_t)across; g.down = (uint32_t)down; g.nc = (uint32_t)nc;
    g.n_ch = w->n_channels; g.per_px = (uint32_t)per_px; g.tiled = tiled ? 1u : 0u; g.comp = w->compression; g.chdr = chdr;
    g.ymin = w->data_window[1]; g.hdr_len = (uint32_t)hdr_len; g.n_images = n_images; g.ncc = (uint32_t)(nc * n_images);
    g.piece_bytes = w->piece_bytes; g.out_align = w->out_align; g.per_p = (uint32_t)per_p;
    zmi_exr_image r;
    memset(&r, 0, sizeof r);
    r.version = 2u | (tiled ? 0x200u : 0u) | (long_names ? 0x400u : 0u);
    r.compression = (uint8_t)w->compression; r.tiled = tiled ? 1u : 0u;
    for (uint32_t k = 0; k < 4u; ++k) { r.data_window[k] = w->data_window[k]; r.display_window[k] = w->display_window[k]; }
    r.width = g.W; r.height = g.H; r.lines_per_chunk = lines; r.tile_w = w->tile_w; r.tile_h = w->tile_h;
    r.n_channels = w->n_channels; r.n_chunks = g.nc; r.row_bytes = (uint32_t)(W * per_px); r.region_bytes = (uint32_t)region;
    r.table_pos = hdr_len;
    static_assert(sizeof r == sizeof g.rec, "zmi_exr_image is 88 bytes");
    memcpy(g.rec, &r, sizeof r);
    h->blob.assign((size_t)w->n_channels * sizeof(zmi_exr_channel), 0u);
    uint64_t off = 0;
    for (uint32_t c = 0; c < w->n_channels; ++c) {
        zmi_exr_channel e;
        off = (off + 3u) & ~3ull;
        e.name_pos = name_pos[c]; e.name_len = (uint32_t)strlen(w->channels[c].name); e.pixel_type = w->channels[c].pixel_type;
        e.x_sampling = e.y_sampling = 1; e.plane_off = (uint32_t)off;
        off += W * H * (e.pixel_type == 1 ? 2u : 4u);
        memcpy(h->blob.data() + (size_t)c * sizeof e, &e, sizeof e);
    }
    h->blob.insert(h->blob.end(), hd.begin(), hd.end());
    h->file_bound = file_bound; h->ppi = ppi; h->ssi = ssi; h->ipi = ipi; h->fpi = fpi;
    h->n_max = (uint32_t)(rows0 * cw0 * (pxr24 ? per_p : per_px));
    return nullptr;
}

extern "C" uint64_t zmi_exr_bound(const zmi_exr_write* w, uint32_t n_images) {
    zmi_xw_host h;
    int level;
    if (zmi_exr_wcheck(w, &level) || zmi_exr_wplan(w, n_images, &h)) return 0;
    const uint64_t am = (uint64_t)w->out_align - 1u;
    return (uint64_t)n_images * ((h.file_bound + am) & ~am);
}

extern "C" int zmi_exr_write_dev(zmi_ctx* c, const zmi_exr_write* w, const void* d_in, const uint64_t* d_in_off, uint32_t n_images, void* d_out,
                                 uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len, uint32_t* d_chunk_len, zmi_exr_image* d_written,
                                 zmi_exr_channel* d_written_channels, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    zmi_xw_host h;
    int level = 0;
    int rc = zmi_exr_wcheck(w, &level);
    if (rc) return rc;
    if (const char* what = zmi_exr_wplan(w, n_images, &h)) return zmi_fail(ZMI_E_ARG, what);
    if (!d_out_off) return zmi_fail(ZMI_E_ARG, "d_out_off is required");
    if ((out_cap && !d_out) || (n_images && (!d_in || !d_in_off || !d_out_len || !d_status))) return zmi_fail(ZMI_E_ARG, "null argument");
    const zmi_xw_plan& g = h.g;
    const int strategy = w->strategy;
    const uint32_t piece_bytes = w->piece_bytes, n = n_images, ncc = g.ncc;
    const bool none = g.comp == 0u;
    const uint64_t np64 = h.ppi * n, scan_bytes = h.ssi * n, items = h.ipi * n;
    if (scan_bytes > (1ull << 44)) return zmi_fail(ZMI_E_NOMEM, "the call's raw bytes size the scratch");
    const uint32_t np = (uint32_t)np64;
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    if (n == 0) {
        ZMI_HIP(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), stream));
        return ZMI_E_OK;
    }

    // launch groups of whole chunks: the pieces the limit (or ZMI_STREAM_GROUP) allows, in units of the largest chunk's pieces; slots
    // and match scratch follow the longest piece there is, the bytes are those of pieces of piece_bytes (zmi_tiff_write_dev)
    const uint32_t max_len = h.n_max < piece_bytes ? h.n_max : piece_bytes;
    const uint64_t pp_max = ((uint64_t)h.n_max + piece_bytes - 1u) / piece_bytes;
    uint64_t stride = 0, gch = ncc, gp = 0;   // a slot; the chunks and the most pieces of a group
    if (!none) {
        stride = zmi_piece_slot_stride(max_len, piece_bytes, level);
        const uint64_t over = zmi_group_override();
        const zmi_group_plan plan = zmi_plan_groups(c->scratch_limit, over, np, max_len, stride);
        gch = plan.group / pp_max;
        if (gch == 0 && over) gch = 1;
        if (gch == 0) return zmi_fail(ZMI_E_NOMEM, "scratch limit too small for one chunk");
        if (gch > ncc) gch = ncc;
        gp = gch * pp_max < np ? gch * pp_max : np;
        rc = zmi_reserve(c->sd_slots, (size_t)(gp * stride));
        if (rc) return rc;
    }
    const uint64_t n_groups = (ncc + gch - 1u) / gch;
    const uint32_t wpg = (uint32_t)((gp + 31u) / 32u);
    const size_t bm_words = none ? 0u : (size_t)(n_groups * wpg);
    const size_t n_rec = (size_t)g.n_ch * sizeof(zmi_exr_channel);

    uint64_t *d_cfirst, *d_soff, *d_item_off, *d_fitem_off, *d_cpos, *d_poff, *d_ppos, *d_run;
    zmi_words4 neff;
    uint32_t *d_csz, *d_cm, *d_fitems, *d_npc, *d_ssz, *d_items, *d_cds, *d_cadler, *d_plen, *d_olen, *d_padler, *d_phead, *d_bad, *d_ends;
    int32_t* d_st;
    uint8_t *d_blob, *d_scan;
    rc = zmi_carve(c->exr, [&](zmi_carver k) {
        k.take(ncc + 1u, d_cfirst, d_soff, d_item_off);   // per chunk: the scans of its pieces, of its room in the scratch, of its items
        k.take(ncc + 1u, d_fitem_off);                    // ... of the trips of its runs (PXR24)
        k.take(ncc, d_cpos);                              // ... its header's place in d_out
        k.take(np, d_poff, d_ppos);                       // per piece: its place in the scratch and in d_out
        k.take(n_groups + 1u, d_run);                     // where every launch group starts in d_out
        k.take(neff);                                     // the chunks that are live: all
        k.take(ncc, d_csz, d_npc, d_ssz, d_items);        // per chunk: raw size, pieces, room, items
        k.take(ncc, d_cm, d_fitems);                      // ... the bytes of its d (PXR24: m, else n), the trips of its runs
        k.take_unless(d_chunk_len, ncc, d_cds);           // ... its dataSize
        k.take(ncc, d_cadler);                            // ... the Adler-32 of its d
        k.take(np, d_plen, d_olen, d_st, d_padler, d_phead);   // per piece: length, encoder's size and status, Adler-32, hole (void: raw chunk)
        k.take(n, d_bad);                                 // per image: the least piece with a status
        k.take(bm_words, d_ends);                         // the bitmap of the pieces that end a chunk's stream
        k.align(8u);
        k.take(h.blob.size(), d_blob);                    // the channel records | the header's bytes
        k.align(256u);
        k.region(d_scan, (size_t)scan_bytes, 64u);        // d of every chunk, each at a multiple of 16
        return k.end();
    });
    if (rc) return rc;
    const zmi_exr_channel* d_chs = (const zmi_exr_channel*)d_blob;
    const uint8_t* in = (const uint8_t*)d_in;

    if (bm_words) ZMI_HIP(hipMemsetAsync(d_ends, 0, bm_words * 4u, stream));
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        for (size_t at = 0; at < h.blob.size(); at += sizeof(zmi_xw_slice::b)) {
            zmi_xw_slice s;
            s.at = at;
            s.len = (uint32_t)(h.blob.size() - at < sizeof s.b ? h.blob.size() - at : sizeof s.b);
            memcpy(s.b, h.blob.data() + at, s.len);
            zmi_launch_exr_wslice(s, d_blob, stream);
        }
        zmi_launch_exr_wchunks(g, d_chs, d_csz, d_npc, d_ssz, d_items, d_cds, neff.w, d_bad, d_run, d_cm, d_fitems, stream);
        zmi_launch_scan_sizes(d_npc, ncc, d_cfirst, stream);
        zmi_launch_scan_sizes(d_ssz, ncc, d_soff, stream);
        zmi_launch_scan_sizes(d_items, ncc, d_item_off, stream);
        if (g.comp == 5u) zmi_launch_scan_sizes(d_fitems, ncc, d_fitem_off, stream);
        if (!none) zmi_launch_exr_wpieces(g, d_cfirst, d_soff, d_cm, (uint32_t)gch, wpg, np, d_poff, d_plen, d_ends, stream);
    }
    if (!none) {
        {
            zmi_scope_timer tm(c, ZMI_K_INFLATE, stream);
            if (g.comp == 5u) zmi_launch_exr_pxr24_forward(g, d_chs, in, d_in_off, d_fitem_off, h.fpi * n, d_soff, d_scan, stream);
            else zmi_launch_exr_zip(g, d_chs, in, d_in_off, d_item_off, items, d_soff, d_scan, stream);
        }
        rc = zmi_piece_checks(c, d_scan, d_poff, d_plen, np, ZMI_WRAP_ZLIB, d_padler, stream);
        if (rc) return rc;
    }
    uint64_t first_piece = 0;
    for (uint64_t grp = 0; grp < n_groups; ++grp) {
        const uint32_t q0 = (uint32_t)(grp * gch), cnt_ch = (uint32_t)(ncc - q0 < gch ? ncc - q0 : gch);
        if (!none) {
            // the pieces in front of chunk q0 + cnt_ch, counted as the device scan counts them: whole images, whole rows of boxes above
            // (never the last row), boxes to the left (never the last column)
            const uint64_t q1 = (uint64_t)q0 + cnt_ch, k1 = q1 % g.nc, tx = k1 % g.across, ty = k1 / g.across;
            const uint64_t last_piece = (q1 / g.nc) * h.ppi + ty * ((g.across - 1u) * h.pp[0][0] + h.pp[1][0]) +
                                        tx * h.pp[0][ty + 1u == g.down ? 1u : 0u];
            const uint32_t cnt = (uint32_t)(last_piece - first_piece);
            rc = zmi_deflate_impl(c, {.d_in = d_scan, .d_in_off = d_poff + first_piece, .d_in_len = d_plen + first_piece, .n = cnt, .max_len = max_len,
                                      .level = level, .strategy = strategy, .wrap = ZMI_WRAP_RAW, .chain_mode = 2u, .d_out = c->sd_slots.p,
                                      .out_stride = stride, .d_out_len = d_olen + first_piece, .d_status = d_st + first_piece, .stream = stream_,
                                      .carry = 0, .ends = d_ends + grp * wpg, .geom_len = piece_bytes});
            if (rc) return rc;
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_exr_wplace(g, q0, cnt_ch, d_cfirst, d_csz, d_olen, d_st, d_run + grp, d_cds, d_cpos, d_ppos, d_phead, d_out_off, d_bad, stream);
            zmi_launch_zip_pack(nullptr, d_poff + first_piece, d_phead + first_piece, (const uint8_t*)c->sd_slots.p, stride, d_olen + first_piece, cnt,
                                stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)stride, (uint8_t*)d_out, d_ppos + first_piece, out_cap, stream);
            first_piece = last_piece;
        } else {
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_exr_wplace(g, q0, cnt_ch, d_cfirst, d_csz, d_olen, d_st, d_run + grp, d_cds, d_cpos, d_ppos, d_phead, d_out_off, d_bad, stream);
        }
    }
    {
        // the chunks that fell back, or all of them: from the planes straight to their place
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_exr_gather(g, d_chs, in, d_in_off, d_item_off, items, d_csz, d_cds, d_cpos, (uint8_t*)d_out, out_cap, stream);
    }
    if (!none) {
        zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
        zmi_launch_combine_segments_adler(d_padler, d_plen, d_cfirst, ncc, neff.w, d_cadler, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_exr_wframe(g, d_blob + n_rec, d_csz, d_cds, d_cpos, d_cadler, d_out_off, (uint32_t)level, (uint32_t)strategy, (uint8_t*)d_out,
                              out_cap, stream);
        zmi_launch_exr_wwords(g, d_chs, d_cds, d_cpos, d_out_off, d_bad, d_st, out_cap, d_out_len, d_status, d_written, d_written_channels, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

static int zmi_host_pipeline_init(zmi_ctx* c) {   // three streams (in / kernels / out) and the events of the two slots
    if (c->hb_live) return 0;
    ZMI_HIP(hipStreamCreateWithFlags(&c->hs_in, hipStreamNonBlocking));
    ZMI_HIP(hipStreamCreateWithFlags(&c->hs_k, hipStreamNonBlocking));
    ZMI_HIP(hipStreamCreateWithFlags(&c->hs_out, hipStreamNonBlocking));
    ZMI_HIP(hipStreamCreateWithFlags(&c->hs_slab, hipStreamNonBlocking));
    for (auto& sl : c->hb) {
        ZMI_HIP(hipEventCreateWithFlags(&sl.in_done, hipEventDisableTiming));
        ZMI_HIP(hipEventCreateWithFlags(&sl.k_done, hipEventDisableTiming));
        ZMI_HIP(hipEventCreateWithFlags(&sl.out_done, hipEventDisableTiming));
    }
    c->hb_live = true;
    return 0;
}
struct zmi_dev_alloc {
    std::vector<void*> ptrs;
    ~zmi_dev_alloc() { for (void* p : ptrs) (void)hipFree(p); }
    void* get(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
};

static int zmi_deflate_batch_simple(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                 int level, int strategy, int wrap, uint8_t* out, uint64_t out_stride, uint32_t* out_len,
                                 int32_t* status) {
    if (!c || (!in && n) || !in_off || !in_len || !out || !out_len || !status) return zmi_fail(ZMI_E_ARG, "null argument");
    if (n == 0) return ZMI_E_OK;
    ZMI_ON_DEVICE(c);
    // pack the shards back to back on the device, 16-byte aligned starts (fast load path)
    std::vector<uint64_t> doff(n);
    uint64_t total = 0;
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        doff[i] = total;
        total += ((uint64_t)in_len[i] + 15u) & ~15ull;
        if (in_len[i] > max_len) max_len = in_len[i];
    }
    if (out_stride % 16u || out_stride < zmi_deflate_bound(max_len, wrap))
        return zmi_fail(ZMI_E_ARG, "out_stride must be a multiple of 16 and >= zmi_deflate_bound(max_len)");
    zmi_dev_alloc A;
    uint8_t* d_in = (uint8_t*)A.get(total + 16);
    uint64_t* d_off = (uint64_t*)A.get((size_t)n * 8);
    uint32_t* d_len = (uint32_t*)A.get((size_t)n * 4);
    uint8_t* d_out = (uint8_t*)A.get((size_t)n * out_stride);
    uint32_t* d_olen = (uint32_t*)A.get((size_t)n * 4);
    int32_t* d_st = (int32_t*)A.get((size_t)n * 4);
    if (!d_in || !d_off || !d_len || !d_out || !d_olen || !d_st) return zmi_fail(ZMI_E_NOMEM, "hipMalloc(batch buffers)");
    for (uint32_t i = 0; i < n;) {   // shards that lie back to back on both sides travel in one copy
        uint32_t j = i;
        uint64_t bytes = in_len[i];
        while (j + 1 < n && in_off[j + 1] == in_off[j] + in_len[j] && doff[j + 1] == doff[j] + in_len[j] && bytes < (1ull << 30)) bytes += in_len[++j];
        if (bytes) ZMI_HIP(hipMemcpy(d_in + doff[i], in + in_off[i], bytes, hipMemcpyHostToDevice));
        i = j + 1;
    }
    ZMI_HIP(hipMemcpy(d_off, doff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    ZMI_HIP(hipMemcpy(d_len, in_len, (size_t)n * 4, hipMemcpyHostToDevice));
    int rc = zmi_deflate_batch_dev(c, d_in, d_off, d_len, n, max_len, level, strategy, wrap, d_out, out_stride, d_olen, d_st,
                                   nullptr);
    if (rc) return rc;
    ZMI_HIP(hipDeviceSynchronize());
    ZMI_HIP(hipMemcpy(out_len, d_olen, (size_t)n * 4, hipMemcpyDeviceToHost));
    ZMI_HIP(hipMemcpy(status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] == 0 && out_len[i])
            ZMI_HIP(hipMemcpy(out + (uint64_t)i * out_stride, d_out + (uint64_t)i * out_stride, out_len[i], hipMemcpyDeviceToHost));
    return ZMI_E_OK;
}


// ---- one host stream decoded as segments (what the stream ABI's inflate() uses for streams with flush points) ----
// A deflate stream that was written with Z_SYNC_FLUSH / Z_FULL_FLUSH points (pigz, this engine's own deflate(): a point every
// 64 KiB of input) carries the marker 00 00 FF FF in front of every byte-aligned restart, and the decode pass needs no window:
// so the pieces between markers can be decoded side by side like the streams of a batch -- thousands of waves instead of
// the one workgroup a single stream gets -- and stitched afterwards (resolve_jump.hip: the back-references of the whole
// output are resolved at once, across segment borders).  `seg_start[0..nseg)` are byte offsets into `in` (ascending,
// seg_start[0] = 0) proposed by the caller, e.g. the bytes behind every marker it found; nothing is taken on trust:
// a segment counts only if the decode of the one before ended exactly at its first byte, on a block boundary, and whatever
// does not check out (a marker that was data, a segment that outgrew its room, a distance that reaches in front of the
// real history) makes the call fall back to the serial decode from there.  Results are those of zmi_inflate_resume on the
// same input: same bytes, status, detail, in_used, resume.
extern "C" int zmi_inflate_resume(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                                  uint32_t hist_len, uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status,
                                  int32_t* detail, uint32_t* in_used, uint32_t* resume);
// Device -> caller's (pageable) memory for the single-stream paths.  hipMemcpy into pageable memory is the runtime's own bounce
// through a small pinned buffer, one thread, 2-4 GB/s: the 15 MiB of a decoded stream took longer to leave the device than to
// decode (measured: 6.4 of 7.5 ms).  Here the bytes go out in 4 MiB pieces through two pinned buffers of the context -- the DMA of
// a piece runs while a few host threads copy the piece before it to where it belongs.  Without pinned memory: the plain copy.
struct zmi_copy_job;
static void zmi_parallel_copy(const std::vector<zmi_copy_job>& jobs, unsigned T);
static int zmi_reserve_pinned(zmi_buf& b, size_t bytes);
static unsigned zmi_host_threads();
static int zmi_d2h(zmi_ctx* c, void* dst, const void* src, size_t n, hipStream_t hs);

// (this function copies asynchronously from vectors and locals of its own frame: an error return must not leave such a copy in
// flight -- the stream is drained first)
#define ZMI_HIPS(call)                                                                  \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) { (void)hipStreamSynchronize(c->host_stream); return zmi_fail(ZMI_E_HIP, #call, e_); } \
    } while (0)
// seg_bit (may be null: all zero): segment j starts at bit seg_bit[j] of byte seg_start[j] -- block boundaries found by the scan
// of zmi_inflate_blocks lie anywhere; in_on_device: c->st_in already holds the stream (that scan has copied it)
static int zmi_split_core(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                          uint32_t hist_len, uint8_t* out, uint32_t out_cap, const uint32_t* seg_start, const uint32_t* seg_bit, uint32_t nseg,
                          bool in_on_device, uint32_t* out_len, int32_t* status, int32_t* detail, uint32_t* in_used, uint32_t* resume,
                          uint32_t* segments_used) {
    if (segments_used) *segments_used = 0;
    if (!c || (!in && in_len) || (!hist && hist_len) || (!out && out_cap) || !out_len || !status || !detail || !in_used || !resume || !seg_start)
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (nseg < 2u || in_bit > 7u || out_cap > (1u << 30) || in_len > 0xFFFFFF00u || seg_start[0] != 0u)
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    for (uint32_t j = 1; j < nseg; ++j)
        if (seg_start[j] <= seg_start[j - 1u] || seg_start[j] >= in_len || (seg_bit && seg_bit[j] > 7u))
            return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    ZMI_ON_DEVICE(c);
    const bool sp_trace = zmi_tune("ZMI_SPLIT_TRACE") != nullptr;
    auto sp_now = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; };
    const double sp_t0 = sp_trace ? sp_now() : 0.0;
    if (hist_len > 32768u) { hist += hist_len - 32768u; hist_len = 32768u; }
    const size_t base = ((size_t)hist_len + 1023u) & ~(size_t)1023u;
    // every segment decodes into a region of its own: 16 bytes of room per compressed byte (a segment that needs more ends the
    // parallel part in front of it)
    std::vector<uint64_t> ioff(nseg), ooff(nseg);
    std::vector<uint32_t> ilen(nseg), ocap(nseg), shist(nseg), sbit(nseg);
    uint64_t scratch = 0;
    for (uint32_t j = 0; j < nseg; ++j) {
        ioff[j] = seg_start[j];
        // (a cut inside a byte: the segment in front of it sees that byte too -- its decode must stop AT the cut, for want of input)
        ilen[j] = (j + 1u < nseg ? seg_start[j + 1u] + ((seg_bit && seg_bit[j + 1u]) ? 1u : 0u) : in_len) - seg_start[j];
        uint64_t room = (uint64_t)ilen[j] * 16u + 4096u;
        if (room > out_cap) room = out_cap;
        ocap[j] = (uint32_t)room;
        ooff[j] = scratch;
        scratch += (room + 1023u) & ~1023ull;
        shist[j] = j == 0u ? hist_len : 32768u;   // (taken on trust by the decode pass, which reads no history; checked at the stitch)
        sbit[j] = j == 0u ? in_bit : (seg_bit ? seg_bit[j] : 0u);
    }
    if (scratch > (3ull << 30)) return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    // (olen .. res travel back in one copy, `one` goes out in one: consecutive takes of one width are contiguous)
    const size_t n = nseg;
    uint64_t *d_ioff, *d_ooff, *d_soff, *d_one_off;
    uint32_t *d_ilen, *d_ocap, *d_hist, *d_bit, *d_olen, *d_used, *d_res, *d_one_len, *d_one_err;
    int32_t *d_st, *d_det;
    const auto meta = [&](zmi_carver k) {
        k.take(n, d_ioff, d_ooff);
        k.take(n + 1, d_soff);                             // where the segments' outputs go in the stitch
        k.take(n, d_ilen, d_ocap, d_hist, d_bit);          // what the host lays out
        k.take(n, d_olen, d_st, d_used, d_det);            // what the decode leaves
        k.take(4 * n, d_res);
        k.take(1, d_one_off);                              // the stitched output as one stream for the jump resolve
        k.take(1, d_one_len, d_one_err);
        k.skip(16u);                                       // (spare: the reservation has always ended with it)
        return k.end();
    };
    const size_t meta_bytes = meta(zmi_carver());
    int rc = zmi_reserve(c->st_in, (size_t)in_len + 64u);
    if (!rc) rc = zmi_reserve(c->st_out, base + (size_t)out_cap + 64u);
    if (!rc) rc = zmi_carve(c->st_meta, meta);
    if (!rc) rc = zmi_reserve(c->sp_out, (size_t)scratch + 64u);
    if (rc) return rc;
    hipStream_t hs = c->host_stream;
    uint8_t* d = (uint8_t*)c->st_meta.p;
    std::vector<uint8_t> hm(meta_bytes, 0);   // the host's image of the tables
    const auto hm_at = [&](const void* dev) { return hm.data() + ((const uint8_t*)dev - d); };
    memcpy(hm_at(d_ioff), ioff.data(), 8 * n); memcpy(hm_at(d_ooff), ooff.data(), 8 * n);
    memcpy(hm_at(d_ilen), ilen.data(), 4 * n); memcpy(hm_at(d_ocap), ocap.data(), 4 * n);
    memcpy(hm_at(d_hist), shist.data(), 4 * n); memcpy(hm_at(d_bit), sbit.data(), 4 * n);
    if (!in_on_device) ZMI_HIPS(hipMemcpyAsync(c->st_in.p, in, in_len, hipMemcpyHostToDevice, hs));
    if (hist_len) ZMI_HIPS(hipMemcpyAsync((uint8_t*)c->st_out.p + base - hist_len, hist, hist_len, hipMemcpyHostToDevice, hs));
    ZMI_HIPS(hipMemcpyAsync(d, hm.data(), meta_bytes, hipMemcpyHostToDevice, hs));
    zmi_inf_scratch dec;   // (the decode's bitmap goes to the stitch below)
    rc = zmi_inflate_impl(c, {.d_in = c->st_in.p, .d_in_off = d_ioff, .d_in_len = d_ilen, .n = nseg,
                              .wrap = ZMI_WRAP_RAW, .d_out = c->sp_out.p, .d_out_off = d_ooff,
                              .d_out_cap = d_ocap, .d_out_hist = d_hist,
                              .d_out_len = d_olen, .d_status = d_st, .d_in_used = d_used,
                              .d_detail = d_det, .d_in_bit = d_bit, .d_resume = d_res,
                              .stream = hs, .decode_only = true, .out_limit = scratch + (1ull << 16), .scratch = &dec});
    if (rc) { (void)hipStreamSynchronize(hs); return rc; }
    std::vector<uint32_t> r(8 * n), codes(nseg, 0u);   // olen | status | used | detail | resume[4n]
    ZMI_HIPS(hipMemcpyAsync(r.data(), d_olen, 32 * n, hipMemcpyDeviceToHost, hs));
    // (every segment's tables' size, see zmi_inflate_resume)
    ZMI_HIPS(hipMemcpyAsync(codes.data(), dec.check, 4u * (size_t)nseg, hipMemcpyDeviceToHost, hs));
    ZMI_HIPS(hipStreamSynchronize(hs));
    const double sp_t1 = sp_trace ? sp_now() : 0.0;
    uint32_t* olen = r.data();
    const uint32_t *used = r.data() + 2 * n, *res = r.data() + 4 * n;
    const int32_t *st = (const int32_t*)(r.data() + n), *det = (const int32_t*)(r.data() + 3 * n);
    // the chain: segment j is CLEAN if its decode ended exactly at its last byte, on a block boundary, with all output complete
    bool trimmed = false;   // a clean segment produced bytes behind its checkpoint: the device copy of the lengths is corrected
    uint32_t tail = 0;   // the first segment that is not clean (or the last one): its result is "the serial decode of the rest"
    std::vector<uint64_t> soff(n + 1, 0);
    uint64_t total = 0;
    for (uint32_t j = 0; j < nseg; ++j) {
        tail = j;
        soff[j] = total;
        // (a cut inside a byte: the decode stops at that bit for want of input, having seen the next block's first bits at most --
        // whatever it made of them lies behind the checkpoint and is dropped)
        const uint32_t cut_byte = j + 1u < nseg ? seg_start[j + 1u] - seg_start[j] : 0u, cut_bit = (j + 1u < nseg && seg_bit) ? seg_bit[j + 1u] : 0u;
        const bool clean = j + 1u < nseg && st[j] == ZMI_BUF_ERROR && det[j] == 1 && res[4 * j] == cut_byte && res[4 * j + 1] == cut_bit &&
                           (cut_bit != 0u || res[4 * j + 2] == olen[j]) && res[4 * j + 2] <= olen[j] && olen[j] <= ocap[j] &&
                           total + res[4 * j + 2] <= out_cap;
        if (!clean) break;
        if (olen[j] != res[4 * j + 2]) { olen[j] = res[4 * j + 2]; trimmed = true; }
        total += olen[j];
    }
    // the tail counts as it stands if it is the stream's real tail (the last segment) or ended the stream; a tail that stopped
    // for any other reason (a marker that was data, no room) is decoded again serially below, from its first byte
    // (and not one that ran out of a region smaller than the room the caller really has left)
    const bool tail_ok = (tail + 1u == nseg || st[tail] == ZMI_OK) && olen[tail] <= ocap[tail] && total + olen[tail] <= out_cap &&
                         (st[tail] == ZMI_OK || (st[tail] == ZMI_BUF_ERROR && (det[tail] == 1 || (det[tail] == 2 && ocap[tail] >= out_cap - total))));
    const uint32_t take = tail + (tail_ok ? 1u : 0u);   // segments whose output is copied
    if (take == 0u || (take == 1u && !tail_ok))        // nothing gained: the serial path
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    if (tail_ok) total += olen[tail] < ocap[tail] ? olen[tail] : ocap[tail];
    soff[take] = total;
    for (uint32_t j = take; j-- > 0u;)   // inflateCodesUsed: the last dynamic block of the part decoded here (a serial tail below overrides it)
        if (codes[j] != 0u) { c->last_codes_used = codes[j]; break; }
    if (total == 0u)
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    // stitch: outputs back to back behind the history, then all back-references at once
    rc = zmi_reserve(c->inf_ptr, (size_t)total * 4u + 512u);
    if (rc) return rc;
    struct { uint64_t off; uint32_t len, err; } one = {0ull, (uint32_t)total, 0u};
    ZMI_HIPS(hipMemcpyAsync(d_soff, soff.data(), 8 * (take + 1u), hipMemcpyHostToDevice, hs));
    ZMI_HIPS(hipMemcpyAsync(d_one_off, &one, sizeof(one), hipMemcpyHostToDevice, hs));
    if (trimmed) ZMI_HIPS(hipMemcpyAsync(d_olen, olen, 4 * (size_t)take, hipMemcpyHostToDevice, hs));
    uint8_t* d_fin = (uint8_t*)c->st_out.p + base;
    zmi_launch_copy_ranges((const uint8_t*)c->sp_out.p, d_ooff, 0, d_olen, take, d_fin,
                           d_soff, total, 0xFFFFFFFFu, hs);
    uint32_t rounds = 2u;   // ceil(log3(total)) + 1
    for (uint64_t span = 3u; rounds < 34u && span < total; span *= 3u) ++rounds;
    {
        zmi_scope_timer tm(c, ZMI_K_RESOLVE, hs);
        zmi_launch_resolve_jump_segments(d_fin, d_soff, take, dec.bitmap, dec.bm_off, (int32_t*)c->inf_ptr.p, total, hist_len, rounds, (uint32_t*)((uint8_t*)c->inf_ptr.p + (size_t)total * 4u),
                                         d_one_err, d_one_off, d_one_len, hs);
    }
    uint32_t err = 0;
    ZMI_HIPS(hipMemcpyAsync(&err, d_one_err, 4, hipMemcpyDeviceToHost, hs));
    double sp_t2 = 0.0;
    if (sp_trace) { ZMI_HIPS(hipStreamSynchronize(hs)); sp_t2 = sp_now(); }
    { const int crc = zmi_d2h(c, out, d_fin, (size_t)total, hs); if (crc) return crc; }
    ZMI_HIPS(hipStreamSynchronize(hs));
    ZMI_HIPS(hipGetLastError());
    if (sp_trace) fprintf(stderr, "[zmi split] %u segments, %u B in, %llu B out: copy-in + decode %.2f ms, stitch + resolve %.2f ms, copy-out %.2f ms\n", nseg, in_len, (unsigned long long)total, sp_t1 - sp_t0, sp_t2 - sp_t1, sp_now() - sp_t2);
    if (err)   // a distance reaches in front of the history that is really there: let the serial decode find and name it
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    if (segments_used) *segments_used = take;
    if (tail_ok) {
        const uint32_t g = (uint32_t)soff[tail];
        *out_len = g + olen[tail];
        *status = st[tail];
        *detail = det[tail];
        *in_used = seg_start[tail] + used[tail];
        resume[0] = seg_start[tail] + res[4 * tail]; resume[1] = res[4 * tail + 1]; resume[2] = g + res[4 * tail + 2]; resume[3] = res[4 * tail + 3];
        return ZMI_E_OK;
    }
    // the clean segments are in `out`; the rest serially, with what has been produced as its history
    const uint32_t at = seg_start[tail], done = (uint32_t)total;
    std::vector<uint8_t> h2;
    if (done >= 32768u) h2.assign(out + done - 32768u, out + done);
    else {
        const uint32_t keep = hist_len < 32768u - done ? hist_len : 32768u - done;
        h2.assign(hist + hist_len - keep, hist + hist_len);
        h2.insert(h2.end(), out, out + done);
    }
    uint32_t ol2 = 0, used2 = 0, res2[4] = {0, 0, 0, 0};
    int32_t st2 = 0, det2 = 0;
    // (a cut found by the block scan lies at a bit: the rest starts there)
    rc = zmi_inflate_resume(c, in + at, in_len - at, tail == 0u ? in_bit : (seg_bit ? seg_bit[tail] : 0u), h2.data(), (uint32_t)h2.size(), out + done,
                            out_cap - done, &ol2, &st2, &det2, &used2, res2);
    if (rc) return rc;
    *out_len = done + ol2; *status = st2; *detail = det2; *in_used = at + used2;
    resume[0] = at + res2[0]; resume[1] = res2[1]; resume[2] = done + res2[2]; resume[3] = res2[3];
    return ZMI_E_OK;
}

#undef ZMI_HIPS
extern "C" int zmi_inflate_split(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                                 uint32_t hist_len, uint8_t* out, uint32_t out_cap, const uint32_t* seg_start, uint32_t nseg,
                                 uint32_t* out_len, int32_t* status, int32_t* detail, uint32_t* in_used, uint32_t* resume,
                                 uint32_t* segments_used) {
    try {
        return zmi_split_core(c, in, in_len, in_bit, hist, hist_len, out, out_cap, seg_start, nullptr, nseg, false, out_len, status, detail,
                              in_used, resume, segments_used);
    } catch (...) { return zmi_fail(ZMI_E_NOMEM, "zmi_inflate_split: out of host memory"); }
}

// One raw deflate stream WITHOUT flush points, decoded as parallel segments all the same: the device looks for the stream's
// dynamic block headers at every bit position (blockscan.hip), the stretches between the boundaries found are decoded side by
// side and stitched as zmi_inflate_split does -- with the same discipline: a cut counts only if the decode in front of it
// ended exactly there.  Results equal zmi_inflate_resume on the same arguments; *segments_used = 0 says the serial path ran
// (too few boundaries found, or the first cut did not check out).
static int zmi_inflate_blocks_body(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist, uint32_t hist_len,
                                   uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status, int32_t* detail, uint32_t* in_used,
                                   uint32_t* resume, uint32_t* segments_used) {
    if (segments_used) *segments_used = 0;
    if (!c || (!in && in_len) || (!hist && hist_len) || (!out && out_cap) || !out_len || !status || !detail || !in_used || !resume)
        return zmi_fail(ZMI_E_ARG, "null argument");
    // (below 256 KiB the scan and the stitch cost more than the serial decode of the few blocks there are)
    uint32_t min_len = 256u << 10, gap = 8192u;
    if (const char* e = zmi_tune("ZMI_BLOCKS_MIN")) { if (atoi(e) > 0) min_len = (uint32_t)atoi(e); }
    if (const char* e = zmi_tune("ZMI_BLOCKS_GAP")) { if (atoi(e) > 0) gap = (uint32_t)atoi(e); }
    if (in_len < min_len || in_bit > 7u || out_cap > (1u << 30) || in_len > (1u << 28))
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    ZMI_ON_DEVICE(c);
    const uint32_t cap = 65536u;
    // stage-1 survivors: one bit position in ~250 of ordinary compressed data; room for one in 64 (more: the scan reports an
    // overflow and the serial decode runs)
    const uint32_t pre_cap = in_len / 8u + 4096u;
    int rc = zmi_reserve(c->st_in, (size_t)in_len + 64u);
    if (!rc) rc = zmi_reserve(c->st_scan, ((size_t)cap + pre_cap) * 4u + 64u);
    if (rc) return rc;
    hipStream_t hs = c->host_stream;
    uint32_t* d_count = (uint32_t*)c->st_scan.p;
    uint32_t* d_list = d_count + 16;
    uint32_t* d_pre = d_list + cap;
    std::vector<uint32_t> found;
    uint32_t count = 0, counts[4] = {0, 0, 0, 0};
    {
        hipError_t e = hipMemcpyAsync(c->st_in.p, in, in_len, hipMemcpyHostToDevice, hs);
        if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, 64, hs);
        if (e != hipSuccess) { (void)hipStreamSynchronize(hs); return zmi_fail(ZMI_E_HIP, "zmi_inflate_blocks: copy-in", e); }
        // (the first block starts at in_bit: it needs no finding; the scan starts behind its header bits)
        zmi_launch_block_scan((const uint8_t*)c->st_in.p, in_len, (uint64_t)in_bit + 3u, d_pre, pre_cap, d_list, cap, d_count, hs);
        e = hipMemcpyAsync(counts, d_count, 16, hipMemcpyDeviceToHost, hs);
        if (e == hipSuccess) e = hipStreamSynchronize(hs);
        if (e != hipSuccess) return zmi_fail(ZMI_E_HIP, "zmi_inflate_blocks: scan", e);
        count = counts[2] ? 0u : counts[0];   // (an incomplete survivor list: nothing is taken from it)
        if (count != 0u && count <= cap) {
            found.resize(count);
            e = hipMemcpyAsync(found.data(), d_list, (size_t)count * 4u, hipMemcpyDeviceToHost, hs);
            if (e == hipSuccess) e = hipStreamSynchronize(hs);
            if (e != hipSuccess) return zmi_fail(ZMI_E_HIP, "zmi_inflate_blocks: list", e);
        }
    }
    std::sort(found.begin(), found.end());
    // cuts: boundaries at least `gap` compressed bytes apart (a segment is one wave's work: it should be worth a wave)
    std::vector<uint32_t> seg_start{0u}, seg_bit{in_bit};
    uint64_t last = 0;
    for (uint32_t pos : found) {
        if ((uint64_t)pos < last + 8ull * gap || (pos >> 3) == 0u) continue;
        seg_start.push_back(pos >> 3);
        seg_bit.push_back(pos & 7u);
        last = pos;
        if (seg_start.size() >= 8192u) break;
    }
    if (zmi_tune("ZMI_SPLIT_TRACE")) fprintf(stderr, "[zmi blocks] %u B: %u of %u stage-1 survivors are block headers, %zu segments\n", in_len, count, counts[3], seg_start.size());
    if (seg_start.size() < 4u)
        return zmi_inflate_resume(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume);
    return zmi_split_core(c, in, in_len, in_bit, hist, hist_len, out, out_cap, seg_start.data(), seg_bit.data(), (uint32_t)seg_start.size(), true,
                          out_len, status, detail, in_used, resume, segments_used);
}
extern "C" int zmi_inflate_blocks(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist, uint32_t hist_len,
                                  uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status, int32_t* detail, uint32_t* in_used,
                                  uint32_t* resume, uint32_t* segments_used) {
    try {
        return zmi_inflate_blocks_body(c, in, in_len, in_bit, hist, hist_len, out, out_cap, out_len, status, detail, in_used, resume, segments_used);
    } catch (...) { return zmi_fail(ZMI_E_NOMEM, "zmi_inflate_blocks: out of host memory"); }
}
// ---- host buffers, pipelined ----
// A caller that hands over host memory pays PCIe both ways (the reference's own caller loop:
// test-libz-rs-sys/examples/blogpost-compress.rs:43-122 -- every real zlib-rs user lives on this path).  Pageable memory is
// the trap: hipMemcpy of pageable memory is the runtime's single-threaded bounce through a small pinned buffer (measured
// round 2: 12-14 GiB/s end to end, with the kernels idle half of the time).  So the batch is cut into chunks that cycle
// through three slots, and per chunk
//   stage in   a few host threads copy the caller's shards into the slot's PINNED staging buffer (memcpy in parallel),
//   H2D        one DMA copy of the whole chunk (stream hs_in),
//   kernels    deflate + zmi_pack_slab_dev: the chunk's compressed streams as one dense slab (stream hs_k),
//   D2H        the slab -- not the compress_bound-strided slots: 0.44 bytes per input byte instead of 1.125 -- into the
//              slot's pinned output staging (stream hs_out),
//   stage out  the host threads scatter the streams to the caller's out + i * out_stride.
// Per chunk the host thread stages chunk k in, hands chunk k-2 out (the slot chunk k is about to use), issues chunk k's
// copies and kernels and chunk k-1's slab copy: the device works on chunks k-1 and k while the host copies.
#include <chrono>
#include <thread>
#include <atomic>
static unsigned zmi_host_threads() {
    unsigned t = std::thread::hardware_concurrency() / 2u;
    t = t < 1u ? 1u : (t > 8u ? 8u : t);
    if (const char* e = zmi_tune("ZMI_HOST_THREADS")) { if (atoi(e) > 0) t = (unsigned)atoi(e) > 64u ? 64u : (unsigned)atoi(e); }
    return t;
}
struct zmi_copy_job { void* dst; const void* src; size_t n; };
// the jobs' bytes split evenly over T threads (the calling thread is one of them)
static void zmi_parallel_copy(const std::vector<zmi_copy_job>& jobs, unsigned T) {
    size_t total = 0;
    for (const zmi_copy_job& j : jobs) total += j.n;
    if (total == 0) return;
    if (T <= 1u || total < ((size_t)4 << 20)) { for (const zmi_copy_job& j : jobs) if (j.n) memcpy(j.dst, j.src, j.n); return; }
    const size_t per = (total + T - 1u) / T;
    auto work = [&](unsigned t) {
        size_t lo = (size_t)t * per, hi = lo + per < total ? lo + per : total, at = 0;
        for (const zmi_copy_job& j : jobs) {
            const size_t a = at, b = at + j.n;
            at = b;
            if (b <= lo || a >= hi) continue;
            const size_t f = a > lo ? a : lo, l = b < hi ? b : hi;
            memcpy((uint8_t*)j.dst + (f - a), (const uint8_t*)j.src + (f - a), l - f);
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (std::thread& x : th) x.join();
}
// gives back the cached staging of the host-buffer pipelines (pinned host memory and the device slots); the streams and events stay
static void zmi_hb_release(zmi_ctx* c) {
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) {
        if (c->hb_pin_in[k].p) { (void)hipHostFree(c->hb_pin_in[k].p); c->hb_pin_in[k] = zmi_buf(); }
        if (c->hb_pin_out[k].p) { (void)hipHostFree(c->hb_pin_out[k].p); c->hb_pin_out[k] = zmi_buf(); }
        if (c->hb_pin_meta[k].p) { (void)hipHostFree(c->hb_pin_meta[k].p); c->hb_pin_meta[k] = zmi_buf(); }
        if (c->hb_slab[k].p) { (void)hipFree(c->hb_slab[k].p); c->hb_slab[k] = zmi_buf(); }
        zmi_ctx::hb_slot& sl = c->hb[k];
        if (sl.in.p) { (void)hipFree(sl.in.p); sl.in = zmi_buf(); }
        if (sl.out.p) { (void)hipFree(sl.out.p); sl.out = zmi_buf(); }
        if (sl.meta.p) { (void)hipFree(sl.meta.p); sl.meta = zmi_buf(); }
    }
}
static size_t zmi_hb_pinned_bytes(const zmi_ctx* c) {
    size_t t = 0;
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) t += c->hb_pin_in[k].cap + c->hb_pin_out[k].cap + c->hb_pin_meta[k].cap;
    return t;
}
// zmi_ctx_trim: a long-lived context that once ran a very large host-buffer batch keeps ~6 GiB of pinned host memory and as much
// HBM for the next one; this hands them back (also done automatically when a call leaves more pinned than the context's limit)
extern "C" int zmi_ctx_trim(zmi_ctx* c) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    ZMI_ON_DEVICE(c);
    zmi_hb_release(c);
    return ZMI_E_OK;
}
extern "C" int zmi_ctx_set_pinned_limit(zmi_ctx* c, uint64_t bytes) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    c->pinned_limit = bytes < (64ull << 20) ? (64ull << 20) : bytes;
    return ZMI_E_OK;
}
// joins the follower thread of a host-buffer pipeline on every way out of its scope -- also when stage_in / the std::thread
// constructor / a vector throws (std::terminate on a joinable thread, and an exception through a C entry point, otherwise)
struct zmi_joiner {
    std::thread& t;
    std::atomic<int>& failed;
    ~zmi_joiner() {
        if (t.joinable()) { failed.store(ZMI_E_NOMEM, std::memory_order_release); t.join(); }
    }
};
static int zmi_d2h(zmi_ctx* c, void* dst, const void* src, size_t n, hipStream_t hs) {
    const size_t CH = (size_t)4 << 20;
    bool bounce = n >= ((size_t)1 << 20);
    if (bounce && (zmi_reserve_pinned(c->st_pin[0], CH) != 0 || zmi_reserve_pinned(c->st_pin[1], CH) != 0)) bounce = false;
    if (bounce && !c->st_pin_ev_live) {
        if (hipEventCreateWithFlags(&c->st_pin_ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->st_pin_ev[1], hipEventDisableTiming) != hipSuccess) bounce = false;
        else c->st_pin_ev_live = true;
    }
    // every error return drains `hs` first: the callers have asynchronous copies into their own frames in flight on it (the
    // `err` word of zmi_split_core), and the DMA into st_pin must not outlive the call either
    if (!bounce) {
        hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, hs);
        const hipError_t es = hipStreamSynchronize(hs);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return zmi_fail(ZMI_E_HIP, "zmi_d2h", e);
        return 0;
    }
    const unsigned T = zmi_host_threads() < 4u ? zmi_host_threads() : 4u;
    const size_t K = (n + CH - 1) / CH;
    for (size_t k = 0; k <= K; ++k) {
        if (k < K) {
            const size_t len = n - k * CH < CH ? n - k * CH : CH;
            hipError_t e = hipMemcpyAsync(c->st_pin[k & 1].p, (const uint8_t*)src + k * CH, len, hipMemcpyDeviceToHost, hs);
            if (e == hipSuccess) e = hipEventRecord(c->st_pin_ev[k & 1], hs);
            if (e != hipSuccess) { (void)hipStreamSynchronize(hs); return zmi_fail(ZMI_E_HIP, "zmi_d2h", e); }
        }
        if (k >= 1) {   // the piece before: wait for its DMA, copy it out (the DMA of piece k runs meanwhile)
            const size_t j = k - 1, len = n - j * CH < CH ? n - j * CH : CH;
            const hipError_t ew = hipEventSynchronize(c->st_pin_ev[j & 1]);
            if (ew != hipSuccess) { (void)hipStreamSynchronize(hs); return zmi_fail(ZMI_E_HIP, "zmi_d2h: hipEventSynchronize", ew); }
            std::vector<zmi_copy_job> jobs{{(uint8_t*)dst + j * CH, c->st_pin[j & 1].p, len}};
            zmi_parallel_copy(jobs, T);
        }
    }
    return 0;
}
static int zmi_reserve_pinned(zmi_buf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) { (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = (bytes + 0xFFFFFull) & ~(size_t)0xFFFFFull;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) { b.p = nullptr; return zmi_fail(ZMI_E_NOMEM, "hipHostMalloc(staging)", e); }
    b.cap = want;
    return 0;
}

static int zmi_deflate_batch_body(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                  int level, int strategy, int wrap, uint8_t* out, uint64_t out_stride, uint32_t* out_len,
                                  int32_t* status);
// (a C entry point: nothing may unwind through it -- the reference builds with panic = abort for the same reason,
// libz-rs-sys-cdylib/src/lib.rs:5-6)
extern "C" int zmi_deflate_batch(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                 int level, int strategy, int wrap, uint8_t* out, uint64_t out_stride, uint32_t* out_len,
                                 int32_t* status) {
    try {
        return zmi_deflate_batch_body(c, in, in_off, in_len, n, level, strategy, wrap, out, out_stride, out_len, status);
    } catch (...) {
        return zmi_fail(ZMI_E_NOMEM, "zmi_deflate_batch: out of host memory (or a thread could not be started)");
    }
}
static int zmi_deflate_batch_body(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                  int level, int strategy, int wrap, uint8_t* out, uint64_t out_stride, uint32_t* out_len,
                                  int32_t* status) {
    if (!c || (!in && n) || !in_off || !in_len || !out || !out_len || !status) return zmi_fail(ZMI_E_ARG, "null argument");
    if (n == 0) return ZMI_E_OK;
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (in_len[i] > max_len) max_len = in_len[i];
    if (out_stride % 16u || out_stride < zmi_deflate_bound(max_len, wrap))
        return zmi_fail(ZMI_E_ARG, "out_stride must be a multiple of 16 and >= zmi_deflate_bound(max_len)");
    // A chunk should fill the chip by itself: one workgroup per shard on 256 CUs wants a few hundred shards per launch (measured:
    // 128-shard chunks made the kernels, not PCIe, the bottleneck; 512 shards of 1 MiB run within 10 % of the per-shard time of
    // the largest launches).  ZMI_HOST_CHUNK (bytes) overrides both bounds (tests).
    // Large batches take larger chunks (an eighth of the input, up to 1 GiB): launches of 512 shards run at 40 GiB/s (two rounds of
    // workgroups on 256 CUs, the slower data classes set the pace), launches of 1024+ at 55-60, above the 46 GiB/s PCIe delivers.
    uint64_t total_in = 0;
    for (uint32_t i = 0; i < n; ++i) total_in += in_len[i];
    uint64_t budget = total_in / 8u;
    budget = budget < (512ull << 20) ? (512ull << 20) : (budget > (1024ull << 20) ? (1024ull << 20) : budget);
    // three slots of pinned staging, each a chunk of input and its worst-case slab (~1.13x): 6.4 chunks in all
    if (budget > c->pinned_limit / 7u) budget = c->pinned_limit / 7u;
    uint32_t min_count = 384u;
    if (const char* e = zmi_tune("ZMI_HOST_CHUNK")) { if (atoll(e) > 0) { budget = (uint64_t)atoll(e); min_count = 1u; } }
    struct chunk { uint32_t first, count; uint64_t bytes; std::vector<uint64_t> doff; };
    std::vector<chunk> chunks;
    for (uint32_t i = 0; i < n;) {
        chunk ck{i, 0, 0, {}};
        while (i < n) {
            const uint64_t a = ((uint64_t)in_len[i] + 15u) & ~15ull;
            if (ck.count >= min_count && ck.bytes + a > budget) break;
            ck.doff.push_back(ck.bytes);
            ck.bytes += a;
            ++ck.count;
            ++i;
        }
        chunks.push_back(std::move(ck));
    }
    const char* pl = zmi_tune("ZMI_HOST_PIPELINE");   // 0: the plain copy-in / kernels / copy-out sequence
    if (chunks.size() < 2 || (pl && !atoi(pl)))
        return zmi_deflate_batch_simple(c, in, in_off, in_len, n, level, strategy, wrap, out, out_stride, out_len, status);
    ZMI_ON_DEVICE(c);
    {
        int irc = zmi_host_pipeline_init(c);
        if (irc) return irc;
    }
    uint64_t max_bytes = 0;
    uint32_t max_count = 0;
    for (const chunk& ck : chunks) { if (ck.bytes > max_bytes) max_bytes = ck.bytes; if (ck.count > max_count) max_count = ck.count; }
    // slab bound: every stream at most out_stride, but never more than the reference's bound for its own length
    uint64_t max_slab = 0;
    for (const chunk& ck : chunks) {
        uint64_t sb = 0;
        for (uint32_t i = 0; i < ck.count; ++i) sb += zmi_deflate_bound(in_len[ck.first + i], wrap) + 16u;
        if (sb > max_slab) max_slab = sb;
    }
    // meta (device and pinned twin): doff u64[count] | in_len u32[count] | out_len u32[count] | status i32[count] | soff u64[count + 1]
    const size_t meta_bytes = (size_t)max_count * 28u + 64u;
    bool zero_copy = true;   // the slab is written into pinned host memory by the pack kernel (0: packed on the device, copied by a copy engine)
    if (const char* zv = zmi_tune("ZMI_HB_ZEROCOPY")) zero_copy = atoi(zv) != 0;
    uint32_t pack_groups = 16u;   // workgroups of the pack kernel that writes to host memory (zmi_launch_copy_ranges_few)
    if (const char* gv = zmi_tune("ZMI_HB_PACK_GROUPS")) { if (atoi(gv) > 0) pack_groups = (uint32_t)atoi(gv); }
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) {
        zmi_ctx::hb_slot& sl = c->hb[k];
        int rc = zmi_reserve(sl.in, (size_t)max_bytes + 64u);
        if (!rc) rc = zmi_reserve(sl.out, (size_t)max_count * out_stride + 64u);
        if (!rc) rc = zmi_reserve(sl.meta, meta_bytes);
        if (!rc && !zero_copy) rc = zmi_reserve(c->hb_slab[k], (size_t)max_slab + 64u);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_in[k], (size_t)max_bytes + 64u);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_out[k], (size_t)max_slab + 64u);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_meta[k], meta_bytes);
        if (rc) {
            // no room for the staging (memlock / container limit, HBM): the plain copy-in / kernels / copy-out sequence needs no
            // pinned memory and a batch that worked before the pipeline existed keeps working
            zmi_hb_release(c);
            return zmi_deflate_batch_simple(c, in, in_off, in_len, n, level, strategy, wrap, out, out_stride, out_len, status);
        }
    }
    const unsigned T = zmi_host_threads();
    const size_t K = chunks.size();
    auto m_doff = [&](void* base) { return (uint64_t*)base; };
    auto m_len = [&](void* base) { return (uint32_t*)((uint8_t*)base + (size_t)max_count * 8u); };
    auto m_olen = [&](void* base) { return (uint32_t*)((uint8_t*)base + (size_t)max_count * 12u); };
    auto m_st = [&](void* base) { return (int32_t*)((uint8_t*)base + (size_t)max_count * 16u); };
    auto m_soff = [&](void* base) { return (uint64_t*)((uint8_t*)base + (size_t)max_count * 20u + 8u - ((size_t)max_count * 20u) % 8u); };
    std::vector<hipEvent_t> sizes_done(ZMI_HB_SLOTS), slab_done(ZMI_HB_SLOTS);
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) {
        ZMI_HIP(hipEventCreateWithFlags(&sizes_done[k], hipEventDisableTiming));
        ZMI_HIP(hipEventCreateWithFlags(&slab_done[k], hipEventDisableTiming));
    }
    struct ev_guard { std::vector<hipEvent_t>& a; std::vector<hipEvent_t>& b; ~ev_guard() { for (hipEvent_t e : a) (void)hipEventDestroy(e); for (hipEvent_t e : b) (void)hipEventDestroy(e); } } evg{sizes_done, slab_done};
    auto stage_in = [&](size_t k) -> int {   // host threads: caller memory -> pinned staging (the slot's previous H2D has finished)
        chunk& ck = chunks[k];
        const int sl = (int)(k % ZMI_HB_SLOTS);
        if (k >= ZMI_HB_SLOTS) ZMI_HIP(hipEventSynchronize(c->hb[sl].in_done));
        std::vector<zmi_copy_job> jobs;
        jobs.reserve(ck.count);
        uint8_t* pin = (uint8_t*)c->hb_pin_in[sl].p;
        for (uint32_t i = 0; i < ck.count; ++i) jobs.push_back({pin + ck.doff[i], in + in_off[ck.first + i], in_len[ck.first + i]});
        zmi_parallel_copy(jobs, T);
        memcpy(m_doff(c->hb_pin_meta[sl].p), ck.doff.data(), (size_t)ck.count * 8u);
        memcpy(m_len(c->hb_pin_meta[sl].p), in_len + ck.first, (size_t)ck.count * 4u);
        return 0;
    };
    auto issue_dev = [&](size_t k) -> int {   // H2D, kernels, pack, sizes back
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        zmi_ctx::hb_slot& sl = c->hb[s2];
        if (k >= ZMI_HB_SLOTS) ZMI_HIP(hipStreamWaitEvent(c->hs_in, sl.k_done, 0));   // the kernels of the chunk that had this slot have read it
        if (k >= ZMI_HB_SLOTS && zero_copy) ZMI_HIP(hipStreamWaitEvent(c->hs_in, slab_done[s2], 0));   // ... and its pack has read the sizes
        ZMI_HIP(hipMemcpyAsync(sl.in.p, c->hb_pin_in[s2].p, (size_t)ck.bytes, hipMemcpyHostToDevice, c->hs_in));
        ZMI_HIP(hipMemcpyAsync(sl.meta.p, c->hb_pin_meta[s2].p, (size_t)max_count * 12u, hipMemcpyHostToDevice, c->hs_in));
        ZMI_HIP(hipEventRecord(sl.in_done, c->hs_in));
        ZMI_HIP(hipStreamWaitEvent(c->hs_k, sl.in_done, 0));
        if (k >= ZMI_HB_SLOTS) ZMI_HIP(hipStreamWaitEvent(c->hs_k, slab_done[s2], 0));   // ... and its slab has left the device
        int rc = zmi_deflate_batch_dev(c, sl.in.p, m_doff(sl.meta.p), m_len(sl.meta.p), ck.count, max_len, level, strategy, wrap, sl.out.p,
                                       out_stride, m_olen(sl.meta.p), m_st(sl.meta.p), c->hs_k);
        if (zero_copy) {
            // The slab does not travel by a copy engine: the pack kernel writes it straight into the pinned host buffer (PCIe
            // writes from the shader, coalesced dwords), on a stream of its own behind the chunk's kernels -- the next chunk's
            // kernels do not wait for it, and the copy engines carry input only.  (Measured: H2D and D2H copies of different
            // streams were served one after the other, a slab queued behind 2.5 GiB of input reached the host 50 ms late.)
            if (rc) return rc;
            ZMI_HIP(hipEventRecord(sl.k_done, c->hs_k));
            ZMI_HIP(hipStreamWaitEvent(c->hs_slab, sl.k_done, 0));
            rc = zmi_scan_sizes_dev(c, m_olen(sl.meta.p), ck.count, m_soff(sl.meta.p), c->hs_slab);
            if (rc) return rc;
            {
                zmi_scope_timer tm(c, ZMI_K_PACK, c->hs_slab);
                zmi_launch_copy_ranges_few((const uint8_t*)sl.out.p, nullptr, out_stride, m_olen(sl.meta.p), ck.count, (uint8_t*)c->hb_pin_out[s2].p,
                                           m_soff(sl.meta.p), c->hb_pin_out[s2].cap, out_stride > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)out_stride,
                                           pack_groups, c->hs_slab);
            }
            ZMI_HIP(hipMemcpyAsync((uint8_t*)c->hb_pin_meta[s2].p + (size_t)max_count * 12u, (uint8_t*)sl.meta.p + (size_t)max_count * 12u,
                                   meta_bytes - (size_t)max_count * 12u, hipMemcpyDeviceToHost, c->hs_slab));
            ZMI_HIP(hipEventRecord(slab_done[s2], c->hs_slab));
            return 0;
        }
        if (!rc) rc = zmi_pack_slab_dev(c, sl.out.p, out_stride, m_olen(sl.meta.p), ck.count, c->hb_slab[s2].p, c->hb_slab[s2].cap,
                                        m_soff(sl.meta.p), c->hs_k);
        if (rc) return rc;
        ZMI_HIP(hipEventRecord(sl.k_done, c->hs_k));
        ZMI_HIP(hipStreamWaitEvent(c->hs_out, sl.k_done, 0));
        // out_len | status | slab offsets travel first: the host needs the slab's size to copy exactly that
        ZMI_HIP(hipMemcpyAsync((uint8_t*)c->hb_pin_meta[s2].p + (size_t)max_count * 12u, (uint8_t*)sl.meta.p + (size_t)max_count * 12u,
                               meta_bytes - (size_t)max_count * 12u, hipMemcpyDeviceToHost, c->hs_out));
        ZMI_HIP(hipEventRecord(sizes_done[s2], c->hs_out));
        return 0;
    };
    auto issue_slab = [&](size_t k) -> int {   // D2H of exactly the slab
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        if (zero_copy) {
            ZMI_HIP(hipEventSynchronize(slab_done[s2]));
            if (m_soff(c->hb_pin_meta[s2].p)[ck.count] > c->hb_pin_out[s2].cap) return zmi_fail(ZMI_E_HIP, "slab larger than its bound");
            return 0;
        }
        ZMI_HIP(hipEventSynchronize(sizes_done[s2]));
        const uint64_t total = m_soff(c->hb_pin_meta[s2].p)[ck.count];
        if (total > c->hb_slab[s2].cap) return zmi_fail(ZMI_E_HIP, "slab larger than its bound");
        // (a stream of its own: hs_out already holds "wait for the kernels of the NEXT chunks" -- the caller's thread runs ahead
        // -- and a slab queued behind those waits left the device only when they had run: 25-29 ms instead of 4)
        if (total) ZMI_HIP(hipMemcpyAsync(c->hb_pin_out[s2].p, c->hb_slab[s2].p, (size_t)total, hipMemcpyDeviceToHost, c->hs_slab));
        ZMI_HIP(hipEventRecord(slab_done[s2], c->hs_slab));
        return 0;
    };
    auto stage_out = [&](size_t k) -> int {   // host threads: pinned slab -> the caller's slots
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        ZMI_HIP(hipEventSynchronize(slab_done[s2]));
        const uint8_t* pm = (const uint8_t*)c->hb_pin_meta[s2].p;
        const uint32_t* ol = m_olen((void*)pm);
        const uint64_t* so = m_soff((void*)pm);
        memcpy(out_len + ck.first, ol, (size_t)ck.count * 4u);
        memcpy(status + ck.first, m_st((void*)pm), (size_t)ck.count * 4u);
        std::vector<zmi_copy_job> jobs;
        jobs.reserve(ck.count);
        const uint8_t* pin = (const uint8_t*)c->hb_pin_out[s2].p;
        for (uint32_t i = 0; i < ck.count; ++i)
            if (m_st((void*)pm)[i] == 0 && ol[i] <= out_stride) jobs.push_back({out + (uint64_t)(ck.first + i) * out_stride, pin + so[i], ol[i]});
        zmi_parallel_copy(jobs, T);
        return 0;
    };
    // Two host threads.  The caller's thread stages chunks in and issues their device work as soon as their slot is free;
    // a second thread follows the results: it waits for a chunk's sizes, issues the copy of exactly its slab, and scatters
    // it.  (One thread doing both waited for results between two issues, and the device idled a third of the time: 18 GiB/s.)
    std::atomic<int> issued{0}, finished{0}, failed{0};
    const int dev_id = c->device;
    const bool hb_trace = zmi_tune("ZMI_HB_TRACE") != nullptr;
    double t_in = 0, t_issue = 0, t_wait_slot = 0, t_slab = 0, t_out = 0, t_wait_issue = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    std::vector<double> tl(K * 6u, 0.0);   // per chunk: stage_in start, end, sizes known, slab arrived, scattered
    const unsigned T_in = T > 1u ? T - T / 3u : 1u, T_out = T > 2u ? T / 3u : 1u;
    auto consumer = [&]() {
        (void)hipSetDevice(dev_id);
        for (size_t k = 0; k < K; ++k) {
            const double a0 = now();
            while (issued.load(std::memory_order_acquire) <= (int)k) {
                if (failed.load(std::memory_order_acquire)) return;
                std::this_thread::yield();
            }
            const double a1 = now();
            int r = issue_slab(k);
            const double a2 = now();
            if (!r && hb_trace) { (void)hipEventSynchronize(slab_done[k % ZMI_HB_SLOTS]); tl[k * 6u + 3u] = now() - t_begin; }
            if (!r) r = stage_out(k);
            tl[k * 6u + 2u] = a2 - t_begin; tl[k * 6u + 4u] = now() - t_begin;
            t_wait_issue += a1 - a0; t_slab += a2 - a1; t_out += now() - a2;
            if (r) { failed.store(r, std::memory_order_release); return; }
            finished.store((int)k + 1, std::memory_order_release);
        }
    };
    (void)T_in; (void)T_out;
    std::thread follower;
    zmi_joiner join_guard{follower, failed};
    follower = std::thread(consumer);
    int rc = 0;
    for (size_t k = 0; k < K && !rc; ++k) {
        while (finished.load(std::memory_order_acquire) + ZMI_HB_SLOTS <= (int)k && !failed.load(std::memory_order_acquire)) std::this_thread::yield();   // slot free
        if (failed.load(std::memory_order_acquire)) break;
        const double b1 = now();
        rc = stage_in(k);
        const double b2 = now();
        if (!rc) rc = issue_dev(k);
        t_wait_slot += 0.0; t_in += b2 - b1; t_issue += now() - b2;
        tl[k * 6u] = b1 - t_begin; tl[k * 6u + 1u] = b2 - t_begin;
        if (!rc) issued.store((int)k + 1, std::memory_order_release);
    }
    const double t_issued_all = now();
    if (rc) failed.store(rc, std::memory_order_release);
    follower.join();
    if (!rc) rc = failed.load();
    // nothing of this call may still be in flight when it returns
    (void)hipStreamSynchronize(c->hs_in);
    (void)hipStreamSynchronize(c->hs_k);
    (void)hipStreamSynchronize(c->hs_out);
    (void)hipStreamSynchronize(c->hs_slab);
    if (hb_trace)
        fprintf(stderr, "[zmi hb] %zu chunks, %u threads: caller stage_in %.1f ms, issue %.1f ms, all issued at %.1f ms; follower waits for issue %.1f, "
                "slab wait+copy-issue %.1f, stage_out %.1f ms; total %.1f ms\n", K, T, t_in, t_issue, t_issued_all - t_begin, t_wait_issue, t_slab, t_out,
                now() - t_begin);
    if (hb_trace)
        for (size_t k = 0; k < K; ++k)
            fprintf(stderr, "[zmi hb]   chunk %zu (%u shards): stage_in %.1f..%.1f, sizes known %.1f, slab on host %.1f, scattered %.1f\n", k, chunks[k].count,
                    tl[k * 6u], tl[k * 6u + 1u], tl[k * 6u + 2u], tl[k * 6u + 3u], tl[k * 6u + 4u]);
    if (zmi_hb_pinned_bytes(c) > c->pinned_limit) zmi_hb_release(c);
    if (rc) return rc;
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

static int zmi_inflate_batch_simple(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                 int wrap, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                 int32_t* status) {
    if (!c || (!in && n) || !in_off || !in_len || !out_off || !out_cap || !out_len || !status)
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (n == 0) return ZMI_E_OK;
    ZMI_ON_DEVICE(c);
    std::vector<uint64_t> dioff(n), dooff(n);
    uint64_t tin = 0, tout = 0;
    for (uint32_t i = 0; i < n; ++i) {
        dioff[i] = tin;
        tin += ((uint64_t)in_len[i] + 15u) & ~15ull;
        dooff[i] = tout;
        tout += ((uint64_t)out_cap[i] + 15u) & ~15ull;
    }
    zmi_dev_alloc A;
    uint8_t* d_in = (uint8_t*)A.get(tin + 16);
    uint8_t* d_out = (uint8_t*)A.get(tout + 16);
    uint64_t* d_ioff = (uint64_t*)A.get((size_t)n * 8);
    uint64_t* d_ooff = (uint64_t*)A.get((size_t)n * 8);
    uint32_t* d_ilen = (uint32_t*)A.get((size_t)n * 4);
    uint32_t* d_ocap = (uint32_t*)A.get((size_t)n * 4);
    uint32_t* d_olen = (uint32_t*)A.get((size_t)n * 4);
    int32_t* d_st = (int32_t*)A.get((size_t)n * 4);
    if (!d_in || !d_out || !d_ioff || !d_ooff || !d_ilen || !d_ocap || !d_olen || !d_st)
        return zmi_fail(ZMI_E_NOMEM, "hipMalloc(batch buffers)");
    for (uint32_t i = 0; i < n; ++i)
        if (in_len[i]) ZMI_HIP(hipMemcpy(d_in + dioff[i], in + in_off[i], in_len[i], hipMemcpyHostToDevice));
    ZMI_HIP(hipMemcpy(d_ioff, dioff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    ZMI_HIP(hipMemcpy(d_ooff, dooff.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    ZMI_HIP(hipMemcpy(d_ilen, in_len, (size_t)n * 4, hipMemcpyHostToDevice));
    ZMI_HIP(hipMemcpy(d_ocap, out_cap, (size_t)n * 4, hipMemcpyHostToDevice));
    // (the capacities are known here: the bitmap scratch is sized exactly)
    int rc = zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = d_ioff, .d_in_len = d_ilen, .n = n, .wrap = wrap, .d_out = d_out, .d_out_off = d_ooff,
                                  .d_out_cap = d_ocap, .d_out_len = d_olen, .d_status = d_st, .out_limit = tout + (1ull << 20), .limit_exact = true});
    if (rc) return rc;
    ZMI_HIP(hipDeviceSynchronize());
    ZMI_HIP(hipMemcpy(out_len, d_olen, (size_t)n * 4, hipMemcpyDeviceToHost));
    ZMI_HIP(hipMemcpy(status, d_st, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n;) {   // outputs that lie back to back on both sides travel in one copy
        if (out_len[i] == 0 || out_len[i] > out_cap[i]) { ++i; continue; }
        uint32_t j = i;
        uint64_t bytes = out_len[i];
        while (j + 1 < n && out_len[j + 1] && out_len[j + 1] <= out_cap[j + 1] && out_off[j + 1] == out_off[j] + out_len[j] &&
               dooff[j + 1] == dooff[j] + out_len[j] && bytes < (1ull << 30))
            bytes += out_len[++j];
        ZMI_HIP(hipMemcpy(out + out_off[i], d_out + dooff[i], bytes, hipMemcpyDeviceToHost));
        i = j + 1;
    }
    return ZMI_E_OK;
}

// Host buffers, pipelined like zmi_deflate_batch: chunks of consecutive streams (by output capacity) cycle through three slots.
// The caller's thread copies a chunk's compressed streams into pinned staging and issues its H2D copy and kernels; the
// decoded bytes leave the device through a copy kernel of a few workgroups that writes straight into pinned host memory
// (PCIe writes from the shader run beside the copy engine's H2D traffic; two copy-engine directions were served one after
// the other, see zmi_deflate_batch), and a second thread scatters every finished chunk into the caller's regions --
// min(out_len, out_cap) bytes of every stream.
static int zmi_inflate_batch_body(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                  int wrap, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                  int32_t* status);
extern "C" int zmi_inflate_batch(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                 int wrap, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                 int32_t* status) {
    try {
        return zmi_inflate_batch_body(c, in, in_off, in_len, n, wrap, out, out_off, out_cap, out_len, status);
    } catch (...) {
        return zmi_fail(ZMI_E_NOMEM, "zmi_inflate_batch: out of host memory (or a thread could not be started)");
    }
}
static int zmi_inflate_batch_body(zmi_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                  int wrap, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                                  int32_t* status) {
    if (!c || (!in && n) || !in_off || !in_len || !out_off || !out_cap || !out_len || !status)
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (n == 0) return ZMI_E_OK;
    // one wave per stream: a launch wants a few thousand streams to keep the chip busy (2048 streams of 1 MiB decode at ~80
    // GiB/s, above what PCIe carries), and a chunk's output has to fit the pinned staging: 2 GiB of capacity per chunk.
    // ZMI_HOST_CHUNK (bytes) overrides both bounds (tests).
    uint64_t budget = 2ull << 30;
    if (budget > c->pinned_limit / 5u) budget = c->pinned_limit / 5u;   // three slots of output staging + their (smaller) input: 4.4 chunks
                                                                         // (the default limit leaves the 2 GiB chunks as they are: a call that
                                                                         // ends above the limit releases the staging, and re-pinning 9 GiB
                                                                         // costs seconds -- measured: 19 -> 3 GiB/s with a limit of 8 GiB)
    uint32_t min_count = 2048u;
    if (const char* e = zmi_tune("ZMI_HOST_CHUNK")) { if (atoll(e) > 0) { budget = (uint64_t)atoll(e); min_count = 1u; } }
    struct chunk { uint32_t first, count; uint64_t in_bytes, out_bytes; std::vector<uint64_t> ioff, ooff; uint32_t max_cap; };
    std::vector<chunk> chunks;
    for (uint32_t i = 0; i < n;) {
        chunk ck{i, 0, 0, 0, {}, {}, 0u};
        while (i < n) {
            const uint64_t ai = ((uint64_t)in_len[i] + 15u) & ~15ull, ao = ((uint64_t)out_cap[i] + 15u) & ~15ull;
            if (ck.count != 0u && (ck.out_bytes + ao > 0xFFFFF000ull || ck.in_bytes + ai > 0xFFFFF000ull)) break;   // (one copy range, u32 length)
            if (ck.count >= min_count && ck.out_bytes + ao > budget) break;
            ck.ioff.push_back(ck.in_bytes);
            ck.ooff.push_back(ck.out_bytes);
            ck.in_bytes += ai;
            ck.out_bytes += ao;
            if (out_cap[i] > ck.max_cap) ck.max_cap = out_cap[i];
            ++ck.count;
            ++i;
        }
        chunks.push_back(std::move(ck));
    }
    const char* pl = zmi_tune("ZMI_HOST_PIPELINE");
    bool fits = true;   // (a chunk leaves the device as one copy range with a 32-bit length)
    for (const chunk& ck : chunks) fits = fits && ck.out_bytes <= 0xFFFFF000ull && ck.in_bytes <= 0xFFFFF000ull;
    if (chunks.size() < 2 || !fits || (pl && !atoi(pl)))
        return zmi_inflate_batch_simple(c, in, in_off, in_len, n, wrap, out, out_off, out_cap, out_len, status);
    ZMI_ON_DEVICE(c);
    int rc = zmi_host_pipeline_init(c);
    if (rc) return rc;
    uint64_t max_in = 0, max_out = 0;
    uint32_t max_count = 0;
    for (const chunk& ck : chunks) {
        if (ck.in_bytes > max_in) max_in = ck.in_bytes;
        if (ck.out_bytes > max_out) max_out = ck.out_bytes;
        if (ck.count > max_count) max_count = ck.count;
    }
    // meta (device and pinned twin): in_off u64 | out_off u64 | in_len | out_cap | out_len | status (u32 each) per stream, then the
    // clamped length min(out_len, out_cap) (what travels back: the decoded bytes, not the capacity)
    const size_t meta_bytes = (size_t)max_count * 36u + 32u;
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) {
        zmi_ctx::hb_slot& sl = c->hb[k];
        rc = zmi_reserve(sl.in, (size_t)max_in + 64u);
        if (!rc) rc = zmi_reserve(sl.out, (size_t)max_out + 64u);
        if (!rc) rc = zmi_reserve(sl.meta, meta_bytes);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_in[k], (size_t)max_in + 64u);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_out[k], (size_t)max_out + 64u);
        if (!rc) rc = zmi_reserve_pinned(c->hb_pin_meta[k], meta_bytes);
        if (rc) {   // as in zmi_deflate_batch: without the staging the plain path still works
            zmi_hb_release(c);
            return zmi_inflate_batch_simple(c, in, in_off, in_len, n, wrap, out, out_off, out_cap, out_len, status);
        }
    }
    auto m_ioff = [&](void* b) { return (uint64_t*)b; };
    auto m_ooff = [&](void* b) { return (uint64_t*)((uint8_t*)b + (size_t)max_count * 8u); };
    auto m_ilen = [&](void* b) { return (uint32_t*)((uint8_t*)b + (size_t)max_count * 16u); };
    auto m_ocap = [&](void* b) { return (uint32_t*)((uint8_t*)b + (size_t)max_count * 20u); };
    auto m_olen = [&](void* b) { return (uint32_t*)((uint8_t*)b + (size_t)max_count * 24u); };
    auto m_st = [&](void* b) { return (int32_t*)((uint8_t*)b + (size_t)max_count * 28u); };
    auto m_clen = [&](void* b) { return (uint32_t*)((uint8_t*)b + (size_t)max_count * 32u); };
    const unsigned T = zmi_host_threads();
    const size_t K = chunks.size();
    std::vector<hipEvent_t> out_done(ZMI_HB_SLOTS);
    for (int k = 0; k < ZMI_HB_SLOTS; ++k) ZMI_HIP(hipEventCreateWithFlags(&out_done[k], hipEventDisableTiming));
    struct ev_guard { std::vector<hipEvent_t>& a; ~ev_guard() { for (hipEvent_t e : a) (void)hipEventDestroy(e); } } evg{out_done};
    uint32_t pack_groups = 16u;
    if (const char* gv = zmi_tune("ZMI_HB_PACK_GROUPS")) { if (atoi(gv) > 0) pack_groups = (uint32_t)atoi(gv); }
    bool dma_out = true;
    if (const char* dv = zmi_tune("ZMI_HB_DMA_OUT")) dma_out = atoi(dv) != 0;
    auto stage_in = [&](size_t k) -> int {   // host threads: caller memory -> pinned staging
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        if (k >= ZMI_HB_SLOTS) ZMI_HIP(hipEventSynchronize(c->hb[s2].in_done));
        std::vector<zmi_copy_job> jobs;
        jobs.reserve(ck.count);
        uint8_t* pin = (uint8_t*)c->hb_pin_in[s2].p;
        for (uint32_t i = 0; i < ck.count; ++i) jobs.push_back({pin + ck.ioff[i], in + in_off[ck.first + i], in_len[ck.first + i]});
        zmi_parallel_copy(jobs, T);
        void* pm = c->hb_pin_meta[s2].p;
        memcpy(m_ioff(pm), ck.ioff.data(), (size_t)ck.count * 8u);
        memcpy(m_ooff(pm), ck.ooff.data(), (size_t)ck.count * 8u);
        memcpy(m_ilen(pm), in_len + ck.first, (size_t)ck.count * 4u);
        memcpy(m_ocap(pm), out_cap + ck.first, (size_t)ck.count * 4u);
        return 0;
    };
    auto issue_dev = [&](size_t k) -> int {
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        zmi_ctx::hb_slot& sl = c->hb[s2];
        if (k >= ZMI_HB_SLOTS) {
            ZMI_HIP(hipStreamWaitEvent(c->hs_in, sl.k_done, 0));      // the kernels of the chunk that had this slot have read its input
            ZMI_HIP(hipStreamWaitEvent(c->hs_in, out_done[s2], 0));   // ... and its copy-out has read the job and the results
        }
        ZMI_HIP(hipMemcpyAsync(sl.in.p, c->hb_pin_in[s2].p, (size_t)ck.in_bytes, hipMemcpyHostToDevice, c->hs_in));
        // (two pieces: the results in the middle of the pinned twin belong to the follower thread until it has read them)
        ZMI_HIP(hipMemcpyAsync(sl.meta.p, c->hb_pin_meta[s2].p, (size_t)max_count * 24u, hipMemcpyHostToDevice, c->hs_in));
        ZMI_HIP(hipEventRecord(sl.in_done, c->hs_in));
        ZMI_HIP(hipStreamWaitEvent(c->hs_k, sl.in_done, 0));
        if (k >= ZMI_HB_SLOTS) ZMI_HIP(hipStreamWaitEvent(c->hs_k, out_done[s2], 0));   // the slot's output has left the device
        int r = zmi_inflate_impl(c, {.d_in = sl.in.p, .d_in_off = m_ioff(sl.meta.p), .d_in_len = m_ilen(sl.meta.p), .n = ck.count, .wrap = wrap,
                                     .d_out = sl.out.p, .d_out_off = m_ooff(sl.meta.p), .d_out_cap = m_ocap(sl.meta.p), .d_out_len = m_olen(sl.meta.p),
                                     .d_status = m_st(sl.meta.p), .stream = c->hs_k,
                                     .out_limit = max_out + (1ull << 20)});   // (the bitmap scratch of the largest chunk for every chunk: not exact)
        if (r) return r;
        ZMI_HIP(hipEventRecord(sl.k_done, c->hs_k));
        ZMI_HIP(hipStreamWaitEvent(c->hs_slab, sl.k_done, 0));
        // How the chunk's bytes travel.  When the chunks decoded so far filled most of their capacity (the usual case: capacities
        // that fit), the whole region leaves as ONE copy by the DMA engine, enqueued here, ahead of time -- 35.6 GiB/s of output
        // against 29.4 for the pack kernel, whose stores leave over PCIe at ~32 GB/s whatever its launch looks like (8 / 16 / 32 /
        // 64 / 256 workgroups: 21.4 / 29.7 / 29.5 / 28.5 / 25.9 GiB/s).  Otherwise -- nothing known yet, or streams that were given
        // much more room than they needed -- range by range through the pack kernel: only the decoded bytes travel.
        // The follower thread keeps the evidence current (stage_out); it is the context's, so a second call starts with it.
        // (Deciding per chunk from its own sizes was built: the copy then cannot be enqueued before the kernels have finished,
        // and a 2 GiB copy enqueued late ran at 27.8 GiB/s.)
        zmi_launch_clamp_lens(m_olen(sl.meta.p), m_ocap(sl.meta.p), ck.count, m_clen(sl.meta.p), c->hs_slab);
        if (dma_out && c->hb_out_tight.load(std::memory_order_acquire) == 1) {
            ZMI_HIP(hipMemcpyAsync(c->hb_pin_out[s2].p, sl.out.p, (size_t)ck.out_bytes, hipMemcpyDeviceToHost, c->hs_slab));
        } else {
            zmi_scope_timer tm(c, ZMI_K_PACK, c->hs_slab);
            // every stream's decoded bytes (min(out_len, out_cap): a stream given four times the room it needs sends a quarter)
            zmi_launch_copy_ranges_few((const uint8_t*)sl.out.p, m_ooff(sl.meta.p), 0, m_clen(sl.meta.p), ck.count, (uint8_t*)c->hb_pin_out[s2].p,
                                       m_ooff(sl.meta.p), c->hb_pin_out[s2].cap, ck.max_cap, pack_groups, c->hs_slab);
        }
        ZMI_HIP(hipMemcpyAsync(m_olen(c->hb_pin_meta[s2].p), m_olen(sl.meta.p), (size_t)max_count * 12u, hipMemcpyDeviceToHost, c->hs_slab));
        ZMI_HIP(hipEventRecord(out_done[s2], c->hs_slab));
        return 0;
    };
    auto stage_out = [&](size_t k) -> int {   // host threads: pinned output -> the caller's regions
        chunk& ck = chunks[k];
        const int s2 = (int)(k % ZMI_HB_SLOTS);
        ZMI_HIP(hipEventSynchronize(out_done[s2]));
        const void* pm = c->hb_pin_meta[s2].p;
        const uint32_t* ol = m_olen((void*)pm);
        memcpy(out_len + ck.first, ol, (size_t)ck.count * 4u);
        memcpy(status + ck.first, m_st((void*)pm), (size_t)ck.count * 4u);
        std::vector<zmi_copy_job> jobs;
        jobs.reserve(ck.count);
        const uint8_t* pin = (const uint8_t*)c->hb_pin_out[s2].p;
        uint64_t decoded = 0;
        for (uint32_t i = 0; i < ck.count; ++i) {
            const uint32_t cap = out_cap[ck.first + i], take = ol[i] < cap ? ol[i] : cap;
            decoded += take;
            if (take) jobs.push_back({out + out_off[ck.first + i], pin + ck.ooff[i], take});
        }
        c->hb_out_tight.store(decoded * 4u >= ck.out_bytes * 3u ? 1 : 0, std::memory_order_release);   // (three quarters of the room used)
        zmi_parallel_copy(jobs, T);
        return 0;
    };
    std::atomic<int> issued{0}, finished{0}, failed{0};
    const int dev_id = c->device;
    auto consumer = [&]() {
        (void)hipSetDevice(dev_id);
        for (size_t k = 0; k < K; ++k) {
            while (issued.load(std::memory_order_acquire) <= (int)k) {
                if (failed.load(std::memory_order_acquire)) return;
                std::this_thread::yield();
            }
            const int r = stage_out(k);
            if (r) { failed.store(r, std::memory_order_release); return; }
            finished.store((int)k + 1, std::memory_order_release);
        }
    };
    std::thread follower;
    zmi_joiner join_guard{follower, failed};
    follower = std::thread(consumer);
    rc = 0;
    for (size_t k = 0; k < K && !rc; ++k) {
        while (finished.load(std::memory_order_acquire) + ZMI_HB_SLOTS <= (int)k && !failed.load(std::memory_order_acquire)) std::this_thread::yield();   // slot free
        if (failed.load(std::memory_order_acquire)) break;
        rc = stage_in(k);
        if (!rc) rc = issue_dev(k);
        if (!rc) issued.store((int)k + 1, std::memory_order_release);
    }
    if (rc) failed.store(rc, std::memory_order_release);
    follower.join();
    if (!rc) rc = failed.load();
    (void)hipStreamSynchronize(c->hs_in);
    (void)hipStreamSynchronize(c->hs_k);
    (void)hipStreamSynchronize(c->hs_slab);
    if (zmi_hb_pinned_bytes(c) > c->pinned_limit) zmi_hb_release(c);
    if (rc) return rc;
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// One host stream through the decode zmi_inflate_resume_dev runs: `in` (raw deflate, starting at bit in_bit of its first byte),
// `hist` = the up to 32 KiB of output in front of it.  The staging buffers belong to the context and are reused,
// a streaming caller pays no allocation per call.  out receives min(*out_len, out_cap) bytes.
extern "C" int zmi_inflate_resume(zmi_ctx* c, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                                  uint32_t hist_len, uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status,
                                  int32_t* detail, uint32_t* in_used, uint32_t* resume) {
    if (!c || (!in && in_len) || (!hist && hist_len) || (!out && out_cap) || !out_len || !status || !detail || !in_used || !resume)
        return zmi_fail(ZMI_E_ARG, "null argument");
    if (in_len > 0xFFFFFF00u || out_cap > 0xFFFF0000u || (in_bit & 0xFE0000F8u) != 0u) return zmi_fail(ZMI_E_ARG, "stream too large for one call");
    ZMI_ON_DEVICE(c);
    if (hist_len > 32768u) { hist += hist_len - 32768u; hist_len = 32768u; }
    const size_t base = ((size_t)hist_len + 1023u) & ~(size_t)1023u;   // the output region stays aligned; the history ends where it starts
    int rc = zmi_reserve(c->st_in, (size_t)in_len + 64u);
    if (!rc) rc = zmi_reserve(c->st_out, base + (size_t)out_cap + 64u);
    if (!rc) rc = zmi_reserve(c->st_meta, 256u);
    if (rc) return rc;
    hipStream_t hs = c->host_stream;
    if (in_len) ZMI_HIP(hipMemcpyAsync(c->st_in.p, in, in_len, hipMemcpyHostToDevice, hs));
    if (hist_len) ZMI_HIP(hipMemcpyAsync((uint8_t*)c->st_out.p + base - hist_len, hist, hist_len, hipMemcpyHostToDevice, hs));
    // meta: in_off u64 | out_off u64 | in_len | out_cap | hist | in_bit || out_len | status | in_used | detail | resume[4]
    struct { uint64_t in_off, out_off; uint32_t in_len, out_cap, hist, in_bit; } m = {0, (uint64_t)base, in_len, out_cap, hist_len, in_bit};
    uint8_t* d = (uint8_t*)c->st_meta.p;
    ZMI_HIP(hipMemcpyAsync(d, &m, sizeof(m), hipMemcpyHostToDevice, hs));
    zmi_inf_scratch dec;
    rc = zmi_inflate_impl(c, {.d_in = c->st_in.p, .d_in_off = (const uint64_t*)d, .d_in_len = (const uint32_t*)(d + 16), .n = 1, .wrap = ZMI_WRAP_RAW,
                              .d_out = c->st_out.p, .d_out_off = (const uint64_t*)(d + 8), .d_out_cap = (const uint32_t*)(d + 20),
                              .d_out_hist = (const uint32_t*)(d + 24), .d_out_len = (uint32_t*)(d + 32), .d_status = (int32_t*)(d + 36),
                              .d_in_used = (uint32_t*)(d + 40), .d_detail = (int32_t*)(d + 44), .d_in_bit = (const uint32_t*)(d + 28),
                              .d_resume = (uint32_t*)(d + 48), .stream = hs, .out_limit = (uint64_t)out_cap + (1ull << 16), .limit_exact = true,
                              .scratch = &dec});
    if (rc) { (void)hipStreamSynchronize(hs); return rc; }
    uint32_t r[8], codes = 0;
    ZMI_HIP(hipMemcpyAsync(r, d + 32, sizeof(r), hipMemcpyDeviceToHost, hs));
    // (a resumable decode leaves its tables' size in `check`)
    ZMI_HIP(hipMemcpyAsync(&codes, dec.check, 4, hipMemcpyDeviceToHost, hs));
    ZMI_HIP(hipStreamSynchronize(hs));   // this stream only: other contexts keep running
    if (codes != 0u) c->last_codes_used = codes;   // (a call that met no dynamic block header keeps the earlier figure)
    *out_len = r[0];
    *status = (int32_t)r[1];
    *in_used = r[2];
    *detail = (int32_t)r[3];
    for (int i = 0; i < 4; ++i) resume[i] = r[4 + i];
    const uint32_t n = r[0] < out_cap ? r[0] : out_cap;
    if (n) {
        const int crc = zmi_d2h(c, out, (const uint8_t*)c->st_out.p + base, n, hs);
        if (crc) return crc;
    }
    return ZMI_E_OK;
}

// ---- single-stream inflate (pigz-style): the inverse of zmi_deflate_stream_dev ------------------------------------------------------
// Per launch group of pieces, all on `stream`, no host synchronisation: layout from the cuts -> decode (raw, 32 KiB of history on
// trust) -> cut verification -> output offsets (scan from the device word the previous group ended at) -> symbolic resolve ->
// window scan (carrying the window into the next group) -> substitute into d_out -> per-piece checks.  Then the combine of the
// checks and the trailer.  Stages and their reasons: inflate.hip, "single-stream inflate"; DESIGN.md section 13.
#define ZMI_SI_CH 1024u       // region granularity (SI_CH in inflate.hip)
#define ZMI_SI_WIN 32768u
#define ZMI_SI_B 64u          // pieces per block of the window scan
#define ZMI_SI_SLACK 4096u
// bits: the cuts are bit offsets (zmi_inflate_stream_bits_dev) -- the pieces' start bits go to the decode, the setup and verify steps
// are the bit forms; everything else is one code path
// ix (zmi_inflate_stream_index_dev; null: nothing more is enqueued): the access points kept while the stream is decoded
struct zmi_si_index { uint64_t span; uint64_t *bit, *out; uint8_t* win; uint32_t cap; uint32_t* n_points; uint64_t* max_gap; };
static int zmi_inflate_stream_body(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                   uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                   int32_t* d_status, int32_t* d_detail, void* stream_, bool bits, const zmi_si_index* ix = nullptr) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    if (n_cuts == 0 || !d_cuts)
        return zmi_fail(ZMI_E_ARG, bits ? "zmi_inflate_stream_bits_dev: at least one cut (the end of the header)"
                                        : "zmi_inflate_stream_dev: at least one cut (the end of the header)");
    if (piece_out_max == 0 || piece_out_max > (1u << 30)) return zmi_fail(ZMI_E_ARG, "piece_out_max must be 1 .. 2^30");
    if ((in_len && !d_in) || (out_cap && !d_out) || !d_out_len || !d_in_used || !d_status || !d_detail) return zmi_fail(ZMI_E_ARG, "null argument");
    if (bits && in_len >= (1ull << 60)) return zmi_fail(ZMI_E_ARG, "in_len must be below 2^60 (bit offsets are 64-bit)");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    const uint64_t stride = ((uint64_t)piece_out_max + ZMI_SI_CH - 1u) & ~(uint64_t)(ZMI_SI_CH - 1u);
    // per piece: decode bytes + symbols + its window + bitmap and tables; per block of the scan: a map and a window
    const uint64_t per = stride * 3u + ZMI_SI_WIN + stride / 8u + 128u + (3u * ZMI_SI_WIN) / ZMI_SI_B + 64u;
    const uint64_t group = zmi_plan_groups_per(c->scratch_limit, zmi_group_override(), n_cuts, per).group;
    if (group == 0) return zmi_fail(ZMI_E_NOMEM, "scratch limit too small for one piece");
    const uint32_t G = (uint32_t)group, nblk = (G + ZMI_SI_B - 1u) / ZMI_SI_B;
    const size_t n = n_cuts, g = G;
    uint64_t *d_off, *d_bad, *d_tail;
    uint32_t *d_len, *d_clen, *d_adler, *d_crc, *d_hdr, *d_chk;
    uint8_t* d_carry;
    int rc = zmi_carve(c->si_meta, [&](zmi_carver k) {   // the call's tables
        k.take(n + 1, d_off);            // the pieces' places in d_out
        k.take(1, d_bad, d_tail);        // the first piece that did not verify, and the tail word (zmi_launch_si_verify)
        k.take(n, d_len, d_clen, d_adler, d_crc);   // per piece: decoded size, that clamped to out_cap, check values
        k.take(4, d_hdr);                // what the header said
        k.take(2, d_chk);                // the combined checks
        k.align(16u);
        k.take(ZMI_SI_WIN, d_carry);     // the window carried into the next group
        return k.end();
    });
    if (rc) return rc;
    uint64_t *g_ioff, *g_ooff;
    uint32_t *g_in, *g_cap, *g_hist, *g_olen, *g_used, *g_bit, *g_res;
    int32_t *g_st, *g_det;
    uint16_t *g_agg, *d_sym;
    uint8_t *g_wst, *g_win, *d_dec;
    rc = zmi_carve(c->si_work, [&](zmi_carver k) {       // one launch group's tables and regions
        k.take(g, g_ioff, g_ooff);       // the decode's request (zmi_inf_req)
        k.take(g, g_in, g_cap, g_hist, g_olen, g_st, g_used, g_det);
        k.take(g, g_bit);                // the start bits (the bit forms)
        k.take(4 * g, g_res);            // the resume words
        k.align(256u);
        k.take((size_t)nblk * ZMI_SI_WIN, g_agg);   // per block of the window scan: a map
        k.take((size_t)nblk * ZMI_SI_WIN, g_wst);   // ... and the window it starts with
        k.take(g * ZMI_SI_WIN, g_win);   // per piece: its window
        k.take(g * stride, d_sym);       // ... its symbols
        k.skip(ZMI_SI_SLACK);
        k.take(g * stride, d_dec);       // ... its decoded bytes
        k.skip(ZMI_SI_SLACK);
        return k.end();
    });
    if (rc) return rc;
    ZMI_HIP(hipMemsetAsync(d_off, 0, 8, stream));
    ZMI_HIP(hipMemsetAsync(d_bad, 0xFF, 8, stream));
    ZMI_HIP(hipMemsetAsync(d_tail, 0, 8, stream));
    ZMI_HIP(hipMemsetAsync(d_chk, 0, 8, stream));
    ZMI_HIP(hipMemsetAsync(d_carry, 0, ZMI_SI_WIN, stream));
    if (ix) {
        ZMI_HIP(hipMemsetAsync(ix->n_points, 0, 4, stream));
        ZMI_HIP(hipMemsetAsync(ix->max_gap, 0, 8, stream));
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_si_header((const uint8_t*)d_in, in_len, (uint32_t)wrap, d_hdr, stream);
    }
    const uint32_t kind = wrap == ZMI_WRAP_ZLIB ? 1u : (wrap == ZMI_WRAP_GZIP ? 2u : (wrap == ZMI_WRAP_AUTO ? 3u : 0u));
    for (uint64_t first = 0; first < n; first += group) {
        const uint32_t cnt = (uint32_t)(n - first < group ? n - first : group);
        const uint32_t f = (uint32_t)first;
        {
            zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
            if (bits) zmi_launch_si_setup_bits(d_cuts, n_cuts, in_len, f, cnt, stride, piece_out_max, g_ioff, g_in, g_ooff, g_cap, g_hist, g_bit, stream);
            else zmi_launch_si_setup(d_cuts, n_cuts, in_len, f, cnt, stride, piece_out_max, g_ioff, g_in, g_ooff, g_cap, g_hist, stream);
        }
        zmi_inf_scratch dec;   // (the decode's bitmap covers one group's regions; the symbolic resolve reads it)
        rc = zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = g_ioff, .d_in_len = g_in, .n = cnt, .wrap = ZMI_WRAP_RAW, .d_out = d_dec,
                                  .d_out_off = g_ooff, .d_out_cap = g_cap, .d_out_hist = g_hist, .d_out_len = g_olen, .d_status = g_st,
                                  .d_in_used = g_used, .d_detail = g_det, .d_in_bit = bits ? g_bit : nullptr, .d_resume = g_res,
                                  .stream = stream_, .decode_only = true, .out_limit = group * stride + (1ull << 16), .scratch = &dec});
        if (rc) return rc;
        {
            zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
            (bits ? zmi_launch_si_verify_bits : zmi_launch_si_verify)(d_cuts, n_cuts, f, cnt, g_in, g_olen, g_st, g_det, g_res, piece_out_max,
                                                                      d_len, d_bad, d_tail, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_scan_sizes_base(d_len + f, cnt, d_off + f, d_off + f, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_RESOLVE, stream);
            zmi_launch_si_resolve(d_dec, stride, d_len + f, piece_out_max, cnt, dec.bitmap, dec.bm_off, d_sym, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_PARSE, stream);   // (the window scan; an inflate call runs no cost parse)
            zmi_launch_si_window_scan(d_sym, stride, d_len + f, cnt, ZMI_SI_B, g_agg, d_carry, g_wst, g_win, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_si_subst(d_sym, stride, d_len + f, d_off + f, g_win, cnt, piece_out_max, f, (uint8_t*)d_out, out_cap, d_bad, stream);
            zmi_launch_si_clamp(d_len + f, d_off + f, cnt, out_cap, d_clen + f, stream);
        }
        if (kind) {
            zmi_scope_timer tm(c, ZMI_K_CHECKSUM, stream);
            zmi_launch_checksum((const uint8_t*)d_out, d_off + f, d_clen + f, cnt, kind, d_adler + f, d_crc + f, stream);
        }
        if (ix) {   // the group's points (the walk goes on from the device words the group before left), then their windows out of g_win
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_ix_select(d_cuts, d_off + f, f, cnt, ix->span, ix->bit, ix->out, ix->cap, ix->n_points, ix->max_gap, stream);
            if (ix->win) zmi_launch_ix_gather(d_cuts, d_off + f, f, cnt, ix->bit, ix->out, ix->n_points, g_win, ix->win, stream);
        }
        ZMI_HIP(hipGetLastError());
    }
    if (kind == 1u || kind == 3u) { rc = zmi_checksum_combine_dev(c, ZMI_WRAP_ZLIB, d_adler, d_clen, 1u, n_cuts, d_chk, nullptr, stream_); if (rc) return rc; }
    if (kind == 2u || kind == 3u) { rc = zmi_checksum_combine_dev(c, ZMI_WRAP_GZIP, d_crc, d_clen, 1u, n_cuts, d_chk + 1, nullptr, stream_); if (rc) return rc; }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_si_final((const uint8_t*)d_in, in_len, d_hdr, d_cuts, bits ? 3u : 0u, d_bad, d_tail, d_off + n, d_chk, d_chk + 1, out_cap, d_status,
                            d_detail, d_out_len, d_in_used, stream);
        if (ix) zmi_launch_ix_final(d_status, d_off + n, ix->out, ix->n_points, ix->max_gap, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}
extern "C" int zmi_inflate_stream_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                      uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                      int32_t* d_status, int32_t* d_detail, void* stream_) {
    return zmi_inflate_stream_body(c, d_in, in_len, wrap, d_cuts, n_cuts, piece_out_max, d_out, out_cap, d_out_len, d_in_used, d_status, d_detail,
                                   stream_, false);
}
extern "C" int zmi_inflate_stream_bits_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                           uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                           int32_t* d_status, int32_t* d_detail, void* stream_) {
    return zmi_inflate_stream_body(c, d_in, in_len, wrap, d_cuts, n_cuts, piece_out_max, d_out, out_cap, d_out_len, d_in_used, d_status, d_detail,
                                   stream_, true);
}


// ---- random access into one stream (include/zmi355.h) ----------------------------------------------------------
// The stream body with an index: per launch group the greedy selection over the group's output offsets and the gather of the selected
// pieces' windows out of the window scan's result; behind the trailer check the closing step, which voids the index of a stream that
// did not verify.
extern "C" int zmi_inflate_stream_index_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                            uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                            int32_t* d_status, int32_t* d_detail, uint64_t span, uint64_t* d_ix_bit, uint64_t* d_ix_out,
                                            void* d_ix_win, uint32_t ix_cap, uint32_t* d_n_points, uint64_t* d_max_gap, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (ix_cap == 0) return zmi_fail(ZMI_E_ARG, "zmi_inflate_stream_index_dev: ix_cap must be at least 1");
    if (!d_ix_bit || !d_ix_out || !d_n_points || !d_max_gap) return zmi_fail(ZMI_E_ARG, "zmi_inflate_stream_index_dev: null index argument");
    if ((uintptr_t)d_ix_win & 15u) return zmi_fail(ZMI_E_ARG, "zmi_inflate_stream_index_dev: d_ix_win must be 16-byte aligned");
    const zmi_si_index ix{span, d_ix_bit, d_ix_out, (uint8_t*)d_ix_win, ix_cap, d_n_points, d_max_gap};
    return zmi_inflate_stream_body(c, d_in, in_len, wrap, d_cuts, n_cuts, piece_out_max, d_out, out_cap, d_out_len, d_in_used, d_status, d_detail,
                                   stream_, true, &ix);
}

// Per launch group of ranges, all on `stream`: plan (one lane per range) -> the points' windows in front of the regions -> decode and
// resolve (raw, from a bit position, history in front: the form zmi_inflate_resume_dev uses) -> got / status and the copy table ->
// the trimmed copy.  Scratch per range: 32 KiB + max_gap + max_len + 514 rounded to 16, an eighth of that as bitmap, 128 bytes of
// tables.
#define ZMI_RG_TAIL 258u   // IX_TAIL, inflate.hip
extern "C" int zmi_inflate_ranges_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, const uint64_t* d_ix_bit, const uint64_t* d_ix_out,
                                      const void* d_ix_win, uint32_t n_points, uint64_t max_gap, const uint64_t* d_lo, const uint32_t* d_len,
                                      uint32_t n_ranges, uint32_t max_len, void* d_out, const uint64_t* d_out_off, uint64_t out_stride,
                                      uint32_t* d_got, int32_t* d_status, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (n_points == 0 || !d_ix_bit || !d_ix_out) return zmi_fail(ZMI_E_ARG, "zmi_inflate_ranges_dev: an index of at least one point");
    if (max_len == 0 || max_len > (1u << 30)) return zmi_fail(ZMI_E_ARG, "zmi_inflate_ranges_dev: max_len must be 1 .. 2^30");
    if (max_gap > (1ull << 30)) return zmi_fail(ZMI_E_ARG, "zmi_inflate_ranges_dev: max_gap must be at most 2^30");
    if (in_len >= (1ull << 60)) return zmi_fail(ZMI_E_ARG, "in_len must be below 2^60 (bit offsets are 64-bit)");
    if ((uintptr_t)d_ix_win & 15u) return zmi_fail(ZMI_E_ARG, "zmi_inflate_ranges_dev: d_ix_win must be 16-byte aligned");
    if (n_ranges == 0) return ZMI_E_OK;
    if ((in_len && !d_in) || !d_lo || !d_len || !d_out || !d_got || !d_status) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    const uint64_t room = ((max_gap + max_len + ZMI_RG_TAIL + 15u) & ~15ull) + 256u;
    const uint64_t rstride = ZMI_SI_WIN + room;
    const uint64_t per = rstride + room / 8u + 128u + 32u;
    uint64_t group = c->scratch_limit / per;
    if (group == 0) return zmi_fail(ZMI_E_NOMEM, "scratch limit too small for one range");
    if (group > n_ranges) group = n_ranges;
    const uint32_t G = (uint32_t)group;
    const size_t g = G;
    uint64_t *g_ioff, *g_ooff, *g_csrc, *g_cdst;
    uint32_t *d_u32, *g_olen, *g_used, *g_clen, *g_res;
    int32_t *g_st, *g_det;
    uint8_t* g_reg;
    int rc = zmi_carve(c->si_work, [&](zmi_carver k) {   // one launch group's tables and regions
        k.take(g, g_ioff, g_ooff);
        k.take(g, g_csrc, g_cdst);       // the trimmed copy: from, to
        k.take(8 * g, d_u32);            // in_n | cap | hist | bit | skip | need | k | pre (rg_tab, inflate.hip)
        k.take(g, g_olen, g_st, g_used, g_det);
        k.take(g, g_clen);               // the trimmed copy's lengths
        k.take(4 * g, g_res);
        k.align(256u);
        k.take(g * rstride, g_reg);      // the regions
        return k.end();
    });
    if (rc) return rc;
    for (uint64_t first = 0; first < n_ranges; first += group) {
        const uint32_t cnt = (uint32_t)(n_ranges - first < group ? n_ranges - first : group);
        const uint32_t f = (uint32_t)first;
        {
            zmi_scope_timer tm(c, ZMI_K_PARSE, stream);   // (plan and history; an inflate call runs no cost parse)
            zmi_launch_rg_plan(d_ix_bit, d_ix_out, n_points, d_ix_win ? 1u : 0u, in_len, max_gap, d_lo, d_len, f, cnt, max_len, rstride,
                               g_ioff, g_ooff, d_u32, G, stream);
            if (d_ix_win) zmi_launch_rg_hist((const uint8_t*)d_ix_win, d_u32, G, cnt, rstride, g_reg, stream);
        }
        rc = zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = g_ioff, .d_in_len = d_u32, .n = cnt, .wrap = ZMI_WRAP_RAW, .d_out = g_reg,
                                  .d_out_off = g_ooff, .d_out_cap = d_u32 + g, .d_out_hist = d_u32 + 2 * g, .d_out_len = g_olen, .d_status = g_st,
                                  .d_in_used = g_used, .d_detail = g_det, .d_in_bit = d_u32 + 3 * g, .d_resume = g_res, .stream = stream_,
                                  .out_limit = group * room + (1ull << 16)});   // (the decode's bitmap covers one group's rooms)
        if (rc) return rc;
        {
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_rg_finish(g_ioff, g_ooff, d_u32, G, g_olen, g_st, g_det, f, cnt, d_out_off, out_stride, d_got, d_status, g_csrc, g_clen,
                                 g_cdst, stream);
            zmi_launch_copy_ranges(g_reg, g_csrc, 0, g_clen, cnt, (uint8_t*)d_out, g_cdst, ~0ull, max_len, stream);
        }
        ZMI_HIP(hipGetLastError());
    }
    return ZMI_E_OK;
}

extern "C" int zmi_stream_find_cuts_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, uint64_t min_gap, uint64_t* d_cuts, uint32_t cap,
                                        uint32_t* d_n_cuts, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    if ((in_len && !d_in) || (cap && !d_cuts) || !d_n_cuts) return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    const uint64_t nseg = (in_len + 4095u) / 4096u;
    int rc = zmi_reserve(c->si_seg, 16u + (size_t)nseg * 4u);
    if (rc) return rc;
    uint32_t* d_hdr = (uint32_t*)c->si_seg.p;
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_si_header((const uint8_t*)d_in, in_len, (uint32_t)wrap, d_hdr, stream);
        zmi_launch_si_find_cuts((const uint8_t*)d_in, in_len, d_hdr, d_hdr + 4, min_gap, d_cuts, cap, d_n_cuts, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// Proposals of cuts for a stream WITHOUT flush points: the bit positions of its dynamic block headers (blockscan.hip), thinned
// greedily to at least min_gap bytes apart, ascending, on the device.  The stream is scanned in windows of 64 MiB, one after the
// other on `stream`; the walk of a window continues the list of the window in front of it.  Scratch (c->si_scan): about 9 / 16 of
// min(in_len, 64 MiB) -- 1 KiB of survivor slots per 2 KiB of a window, 4 B of list per 64 B -- whatever in_len is.
extern "C" int zmi_stream_find_blocks_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, int wrap, uint64_t min_gap, uint64_t* d_cuts, uint32_t cap,
                                          uint32_t* d_n_cuts, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (wrap < ZMI_WRAP_RAW || wrap > ZMI_WRAP_AUTO) return zmi_fail(ZMI_E_ARG, "wrap must be raw/zlib/gzip/auto");
    if ((in_len && !d_in) || (cap && !d_cuts) || !d_n_cuts) return zmi_fail(ZMI_E_ARG, "null argument");
    if (in_len >= (1ull << 60) || min_gap >= (1ull << 60)) return zmi_fail(ZMI_E_ARG, "in_len and min_gap must be below 2^60 (bit offsets are 64-bit)");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    uint64_t window = 64ull << 20;   // (positions inside a window are 32-bit: at most 2^28 bytes)
    if (const char* wv = zmi_tune("ZMI_BLOCKS_WINDOW")) if (atoll(wv) >= 64 && atoll(wv) <= (1ll << 28)) window = (uint64_t)atoll(wv);
    const uint64_t widest = in_len < window ? in_len : window;
    const size_t nb = zmi_block_scan_groups((uint32_t)(8u * widest)), slot = zmi_block_scan_slot();
    const uint32_t vcap = (uint32_t)(widest / 64u) + 1024u;
    // hdr u32[4] | voff u64[nb + 1] | cnt u32[nb] | vcnt u32[nb] | vlist u32[vcap] | slots u32[nb * slot]
    const size_t s_hdr = 0, s_voff = 16, s_cnt = s_voff + 8 * (nb + 1), s_vcnt = s_cnt + 4 * nb, s_vlist = s_vcnt + 4 * nb,
                 s_slots = s_vlist + 4 * (size_t)vcap, bytes = s_slots + 4 * nb * slot;
    int rc = zmi_reserve(c->si_scan, bytes);
    if (rc) return rc;
    uint8_t* S = (uint8_t*)c->si_scan.p;
    uint32_t* d_hdr = (uint32_t*)(S + s_hdr);
    const uint64_t gap_bits = 8ull * (min_gap ? min_gap : 1u);
    zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
    zmi_launch_si_header((const uint8_t*)d_in, in_len, (uint32_t)wrap, d_hdr, stream);
    uint64_t base = 0;
    do {
        const uint64_t own = in_len - base < window ? in_len - base : window;
        const uint64_t vis = in_len - base < window + zmi_block_scan_look() ? in_len - base : window + zmi_block_scan_look();
        zmi_launch_block_scan_window((const uint8_t*)d_in + base, (uint32_t)vis, 8ull * base, (uint32_t)(8u * own), d_hdr, (uint32_t*)(S + s_slots),
                                     (uint32_t*)(S + s_cnt), (uint32_t*)(S + s_vcnt), (uint64_t*)(S + s_voff), (uint32_t*)(S + s_vlist), vcap,
                                     gap_bits, base == 0 ? 1u : 0u, d_cuts, cap, d_n_cuts, stream);
        base += own;
    } while (base < in_len);
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

// ---- multi-member gzip files: one scan for the member starts, one call that decodes every member in place ----------------------------
// pack.hip (the scan) and inflate.hip ("multi-member gzip files") hold the kernels and their reasons; DESIGN.md section 16.
extern "C" int zmi_gzip_find_members_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, uint64_t* d_starts, uint32_t cap, uint32_t* d_n_starts,
                                         void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if ((in_len && !d_in) || (cap && !d_starts) || !d_n_starts) return zmi_fail(ZMI_E_ARG, "null argument");
    if (in_len >= (1ull << 45)) return zmi_fail(ZMI_E_ARG, "in_len must be below 2^45");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    if (in_len == 0) { ZMI_HIP(hipMemsetAsync(d_n_starts, 0, 4, stream)); return ZMI_E_OK; }
    const size_t nseg = zmi_mm_scan_segments(in_len, (uint32_t)((uintptr_t)d_in & 15u));
    int rc = zmi_reserve(c->mm_scan, 8u * (nseg + 1u) + 4u * nseg);
    if (rc) return rc;
    uint64_t* d_off = (uint64_t*)c->mm_scan.p;
    {
        zmi_scope_timer tm(c, ZMI_K_PACK, stream);
        zmi_launch_mm_find((const uint8_t*)d_in, in_len, (uint32_t*)(d_off + nseg + 1u), d_off, d_starts, cap, d_n_starts, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}

extern "C" int zmi_inflate_members_dev(zmi_ctx* c, const void* d_in, uint64_t in_len, const uint64_t* d_starts, uint32_t n_starts, void* d_out,
                                       uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used, uint32_t* d_members, uint64_t* d_member_off,
                                       int32_t* d_status, int32_t* d_detail, void* stream_) {
    if (!c) return zmi_fail(ZMI_E_ARG, "null context");
    if (!d_out_len || !d_in_used || !d_members || !d_status || !d_detail || (in_len && !d_in) || (out_cap && !d_out))
        return zmi_fail(ZMI_E_ARG, "null argument");
    hipStream_t stream = (hipStream_t)stream_;
    ZMI_ON_DEVICE(c);
    if (in_len == 0) {   // no input: no members
        ZMI_HIP(hipMemsetAsync(d_out_len, 0, 8, stream));
        ZMI_HIP(hipMemsetAsync(d_in_used, 0, 8, stream));
        ZMI_HIP(hipMemsetAsync(d_members, 0, 4, stream));
        ZMI_HIP(hipMemsetAsync(d_status, 0, 4, stream));
        ZMI_HIP(hipMemsetAsync(d_detail, 0, 4, stream));
        if (d_member_off) ZMI_HIP(hipMemsetAsync(d_member_off, 0, 8, stream));
        return ZMI_E_OK;
    }
    if (n_starts == 0 || !d_starts) return zmi_fail(ZMI_E_ARG, "zmi_inflate_members_dev: at least one start (offset 0)");
    // Launch groups: the decode keeps one bit of scratch per byte of output capacity, and all regions of a call lie inside out_cap.
    // An out_cap above the scratch limit is cut at multiples of half the limit: group g holds the members whose planned offset lies
    // in [g * half, (g + 1) * half) -- the members come from device words, so every group is a launch over all proposals in which
    // the others are empty streams.  Offsets and bytes do not depend on the cut.  The limit is the context's scratch limit alone
    // (as zmi_inflate_stream_dev): the inflate-out limit is the setting for batch calls that size no scratch of their own and says nothing here.
    uint64_t limit = c->scratch_limit;
    if (const char* lv = zmi_tune("ZMI_MM_LIMIT")) if (atoll(lv) >= (128ll << 10)) limit = (uint64_t)atoll(lv);   // (tests: groups on small files)
    uint64_t half = 0, groups = 1, room_max = ~0ull;
    if (out_cap > limit) {
        half = limit / 2u;
        groups = out_cap / half + 1u;
        if (groups > 65536u) return zmi_fail(ZMI_E_NOMEM, "scratch limit too small for this out_cap (more than 65536 launch groups)");
        room_max = limit;   // (the last resort decodes one member alone: the whole bitmap is its)
    }
    uint32_t repairs = ZMI_MM_REPAIR_PASSES;
    if (const char* rv = zmi_tune("ZMI_MM_REPAIR")) repairs = (uint32_t)atoi(rv);   // (the probe: what do the idle passes cost?)
    const size_t n = n_starts;
    uint64_t *l_ioff, *l_ooff, *d_off, *d_rank, *g_ioff, *g_ooff;
    uint32_t *d_w, *l_in, *l_cap, *l_olen, *l_used, *d_tab, *g_in, *g_cap, *g_olen, *g_used;
    int32_t *l_st, *l_det, *g_st, *g_det;
    int rc = zmi_carve(c->mm_meta, [&](zmi_carver k) {
        k.take(16, d_w);             // the call's words
        k.take(1, l_ioff, l_ooff);   // the last resort's launch of one member
        k.take(1, l_in, l_cap, l_olen, l_st, l_used, l_det);
        k.skip(24u);                 // (spare: the per-member tables have always started at byte 128)
        k.take(n + 1, d_off);        // the members' planned places in d_out
        k.take(n + 1, d_rank);       // the scan of the live flags
        k.take(n, g_ioff, g_ooff);   // a launch group: one stream per proposal
        k.take(8 * n, d_tab);        // the proposals' tables (mm_tab, inflate.hip)
        k.take(n, g_in, g_cap, g_olen, g_st, g_used, g_det);
        return k.end();
    });
    if (rc) return rc;
    const uint64_t bm_limit = (out_cap > limit ? limit : out_cap) + (1ull << 16);   // the decode's bitmap covers one group's regions
    ZMI_HIP(hipMemsetAsync(d_w, 0, 64, stream));
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_mm_init(d_starts, n_starts, in_len, d_tab, d_off, d_w, stream);
    }
    for (uint32_t pass = 0; pass <= repairs; ++pass) {
        {
            zmi_scope_timer tm(c, ZMI_K_PARSE, stream);   // (class 5: the plan; an inflate call runs no cost parse)
            zmi_launch_mm_plan(d_starts, n_starts, d_tab, d_off, d_w, (const uint8_t*)d_in, in_len, pass, stream);
        }
        {
            zmi_scope_timer tm(c, ZMI_K_PACK, stream);
            zmi_launch_scan_sizes(d_tab + 2 * n, n_starts, d_off, stream);   // (the planned sizes)
        }
        for (uint64_t g = 0; g < groups; ++g) {
            {
                zmi_scope_timer tm(c, ZMI_K_PARSE, stream);
                zmi_launch_mm_setup(d_starts, n_starts, d_tab, d_off, d_w, out_cap, half, (uint32_t)g, g_ioff, g_in, g_ooff, g_cap, stream);
            }
            rc = zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = g_ioff, .d_in_len = g_in, .n = n_starts, .wrap = ZMI_WRAP_GZIP, .d_out = d_out,
                                      .d_out_off = g_ooff, .d_out_cap = g_cap, .d_out_len = g_olen, .d_status = g_st, .d_in_used = g_used,
                                      .d_detail = g_det, .stream = stream_, .out_limit = bm_limit});
            if (rc) return rc;
            zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
            zmi_launch_mm_collect(d_starts, n_starts, d_tab, d_off, d_w, out_cap, half, (uint32_t)g, g_olen, g_st, g_used, g_det, stream);
        }
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_mm_verify(d_starts, n_starts, d_tab, d_off, d_w, out_cap, pass, pass < repairs ? 1 : 0, stream);
    }
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_mm_lr_setup(d_starts, n_starts, d_tab, d_off, d_w, in_len, out_cap, room_max, l_ioff, l_in, l_ooff, l_cap, stream);
    }
    zmi_inf_scratch lr;   // (of the last-resort launch)
    rc = zmi_inflate_impl(c, {.d_in = d_in, .d_in_off = l_ioff, .d_in_len = l_in, .n = 1u, .wrap = ZMI_WRAP_GZIP, .d_out = d_out, .d_out_off = l_ooff,
                              .d_out_cap = l_cap, .d_out_len = l_olen, .d_status = l_st, .d_in_used = l_used, .d_detail = l_det, .stream = stream_,
                              .no_jump = true, .out_limit = bm_limit, .scratch = &lr});
    if (rc) return rc;
    {
        zmi_scope_timer tm(c, ZMI_K_VERIFY, stream);
        zmi_launch_scan_sizes(d_tab, n_starts, d_rank, stream);   // (the live flags)
        zmi_launch_mm_final(d_starts, n_starts, d_tab, d_off, d_w, (const uint8_t*)d_in, in_len, out_cap, d_rank, l_olen, l_st, l_used, l_det, lr.check,
                            lr.crc, d_out_len, d_in_used, d_members, d_member_off, d_status, d_detail, stream);
    }
    ZMI_HIP(hipGetLastError());
    return ZMI_E_OK;
}
