// zmi_scratch.h -- host helpers of zmi_api.hip that need no HIP type: the carver that lays a call's device tables out in one
// context buffer, and the plan of the launch groups of the deflate-side calls.  Plain C++17; tests/c/scratch_selftest.cpp
// compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef ZMI_EMU
#include <assert.h>
#endif

// Four u32 words that several kernels share as one 16-byte block (cleared by one memset): word 0 is a count, word 1 a call-wide
// status, and the upper half is read as one u64 sum by the layout kernels.  The block is 8-byte aligned for that u64.
struct zmi_words4 {
    uint32_t* w = nullptr;
    uint32_t* word(unsigned i) const { return w + i; }
    uint64_t* upper64() const { return (uint64_t*)(w + 2); }
};

// Hands out consecutive typed arrays from one buffer.  A layout is written once, as a function of a carver, and run twice: on a
// carver without a base (the sizing pass: the pointers it yields are null, end() is the number of bytes to reserve), then on the
// reserved buffer.  Every take is aligned for its element type, so consecutive takes of one type are contiguous.  The emulator
// build asserts on every take that the carving pass stays within the capacity it was given; the product build carries no check.
struct zmi_carver {
    uint8_t* base = nullptr;
    size_t at = 0, cap = 0;
    zmi_carver() = default;
    zmi_carver(void* p, size_t capacity) : base((uint8_t*)p), cap(capacity) {}

    size_t end() const { return at; }
    void align(size_t a) { at = (at + a - 1u) & ~(a - 1u); }   // a: a power of two
    // one array of `count` elements for every pointer named, in that order
    template <class T, class... More> void take(size_t count, T*& p, More*&... more) {
        align(alignof(T));
        p = base ? (T*)(base + at) : nullptr;
        skip(count * sizeof(T));
        if constexpr (sizeof...(more) != 0) take(count, more...);
    }
    // a table the call owns unless the caller supplies one of its own to stand in for it (which then takes no room here)
    template <class T> void take_unless(T* supplied, size_t count, T*& p) {
        if (supplied) p = supplied;
        else take(count, p);
    }
    void take(zmi_words4& b) {
        align(8u);
        take(4u, b.w);
    }
    // bytes behind the tables with `margin` bytes clear on either side (kernels that load whole dwords or lines around their data)
    void region(uint8_t*& p, size_t bytes, size_t margin) {
        skip(margin);
        take(bytes, p);
        skip(margin);
    }
    void skip(size_t bytes) {
        at += bytes;
#ifdef ZMI_EMU
        assert(!base || at <= cap);
#endif
    }
};

// The launch groups of a deflate-side call: `group` pieces share one launch, so that a group's output slots (slot_stride bytes per
// piece) and the encoder's match scratch (per_piece bytes per piece) together stay within the scratch limit.  override_group
// (ZMI_STREAM_GROUP; 0: none) replaces the quotient.  group = 0: the limit is too small for one piece (np = 0 is also no group, and
// no failure: the caller tells them apart).  wpg, n_groups, bm_words: the geometry of the one-bit-per-piece bitmaps, one row of
// wpg words per group.
struct zmi_group_plan {
    uint64_t group = 0, n_groups = 0;
    uint32_t wpg = 0;
    size_t bm_words = 0;
};
inline zmi_group_plan zmi_plan_groups_per(uint64_t scratch_limit, uint64_t override_group, uint64_t np, uint64_t per_piece) {
    zmi_group_plan p;
    uint64_t group = per_piece ? scratch_limit / per_piece : np;   // (nothing per piece: one group)
    if (override_group) group = override_group;
    if (group > np) group = np;
    if (group == 0) return p;
    p.group = group;
    p.wpg = (uint32_t)((group + 31u) / 32u);
    p.n_groups = (np + group - 1u) / group;
    p.bm_words = (size_t)(p.n_groups * p.wpg);
    return p;
}
// ... where a piece costs its slot and the match scratch of max_len input bytes: 4 bytes per position of the length rounded up to
// 64 (64 at least), and a sixteenth of that again
inline uint64_t zmi_match_per(uint64_t max_len) {
    const uint64_t padded = (max_len + 63u) & ~63ull;
    return (padded ? padded : 64u) * 4u;
}
inline zmi_group_plan zmi_plan_groups(uint64_t scratch_limit, uint64_t override_group, uint64_t np, uint64_t max_len, uint64_t slot_stride) {
    const uint64_t match_per = zmi_match_per(max_len);
    return zmi_plan_groups_per(scratch_limit, override_group, np, slot_stride + match_per + match_per / 16u);
}
