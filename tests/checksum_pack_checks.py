"""Exact checks of the kernels that decide whether a finished stream is accepted: zmi_checksum_kernel and zmi_combine_kernel
(csrc/checksum.hip), zmi_scan_sizes_kernel, zmi_copy_ranges_kernel and zmi_frame_kernel (csrc/pack.hip), zmi_stitch_plan_kernel
(csrc/exchange.hip).  Shared by the emulator tests (CPU, tests/test_emu_checksum_pack.py) and the -m gpu tests
(tests/test_gpu_checksum_pack.py): the same inputs go through the library and through a plain host reference, and every
comparison is equality.

A target is an object with these methods, all on host numpy arrays (the adapter moves them to where the library reads them):
  checksums(buf u8, launches) -> (address of buf[0] as the library sees it, [(adler u32[n], crc u32[n]) per launch]);
      a launch is (off u64[n], len u32[n], kind, adler_init u32[n], crc_init u32[n]): the result arrays start as the *_init
  combine(checks u32, lens u32, wrap, world) -> (check, total length) as Python ints
  scan_sizes(lens u32[n]) -> u64[n + 1]
  stitch_plan(table u32[world, n_local]) -> (goff u64[world, n_local], soff u64[world, n_local + 1], totals list of world + 1)
  copy_ranges(src u8, src_off u64[n] or None, src_stride, lens u32[n], max_len, dst u8, dst_off u64[n], dst_cap)
      -> (address of src[0], address of dst[0], dst after the call); the library is told dst_cap bytes of room
  pack_slab(slots u8[n, stride], lens u32[n], slab u8) -> (address of slots[0, 0], slab after the call, offsets u64[n + 1])
  frame(out u8, cap, payload_len, check, raw_len, wrap, level, strategy) -> (out after the call, reported length, status)
"""
import struct
import zlib

import numpy as np

BASE = 65521
POLY = 0xEDB88320


# ---- host references -----------------------------------------------------------------------------------------------------
def gf2_mulmod(a, b):
    """a(x) * b(x) mod P in the reflected bit order of CRC-32 (bit 31 is x^0, P = x^32 + ... as 0xEDB88320)"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def gf2_xpow8(nbytes):
    """x^(8 * nbytes) mod P"""
    r, pw = 0x80000000, 0x00800000   # x^0, x^8
    while nbytes:
        if nbytes & 1:
            r = gf2_mulmod(r, pw)
        pw = gf2_mulmod(pw, pw)
        nbytes >>= 1
    return r


def crc32_combine(c1, c2, len2):
    """CRC-32 of A || B from crc(A), crc(B), len(B): the conditioning (initial value and final inversion, both 0xFFFFFFFF) cancels,
    what is left is crc(A) moved len(B) bytes forward -- a multiplication by x^(8 * len(B)) -- plus crc(B)"""
    return gf2_mulmod(c1, gf2_xpow8(len2)) ^ c2


def adler32_combine(a1, a2, len2):
    """RFC 1950: s1 = 1 + sum of the bytes, s2 = sum of the s1 after every byte (mod 65521).  Behind A, every one of B's len2
    running s1 values is larger by s1(A) - 1, and s2 starts from s2(A) instead of 0."""
    s1a, s2a, s1b, s2b = a1 & 0xFFFF, a1 >> 16, a2 & 0xFFFF, a2 >> 16
    s1 = (s1a + s1b - 1) % BASE
    s2 = (s2a + s2b + (len2 % BASE) * (s1a - 1)) % BASE
    return (s2 << 16) | s1


def logical_order(world, n_local):
    """table index of logical entry g of a rank-major table [world, n_local]: entry [r, j] is piece j * world + r"""
    g = np.arange(world * n_local, dtype=np.int64)
    return (g % world) * n_local + g // world


def fold_scalar(checks, lens, wrap):
    """the check value and length of the concatenation of the entries in the order given, one combine call per entry; an entry of
    length 0 is nothing, whatever its check field holds"""
    comb = adler32_combine if wrap == 1 else crc32_combine
    acc, total = (1 if wrap == 1 else 0), 0
    for c, l in zip(checks, lens):
        c, l = int(c), int(l)
        if l:
            acc = comb(acc, c, l)
            total += l
    return acc, total


_MULK_TABLES = {}


def _mulk_tables(k):
    """multiplication by the constant x^(8 * 2^k) is linear in the other factor: four byte tables, from the 32 products of single bits"""
    if k not in _MULK_TABLES:
        kk = gf2_xpow8(1 << k)
        cols = [gf2_mulmod(1 << j, kk) for j in range(32)]
        tabs = np.zeros((4, 256), dtype=np.uint32)
        for byte in range(4):
            for bit in range(8):
                step = 1 << bit
                tabs[byte, step:2 * step] = tabs[byte, :step] ^ np.uint32(cols[8 * byte + bit])
        _MULK_TABLES[k] = tabs
    return _MULK_TABLES[k]


def fold_crc_vector(checks, lens):
    """the same CRC fold without a loop over the entries: crc(A1 || ... || An) = xor of crc(Ai) * x^(8 * bytes behind Ai)"""
    lens = np.asarray(lens, dtype=np.uint64)
    keep = lens != 0
    c = np.asarray(checks, dtype=np.uint32)[keep].copy()
    l = lens[keep]
    if l.size == 0:
        return 0, 0
    behind = (np.cumsum(l[::-1])[::-1] - l).astype(np.uint64)
    for k in range(int(behind.max()).bit_length()):
        t = _mulk_tables(k)
        moved = t[0][c & 0xFF] ^ t[1][(c >> 8) & 0xFF] ^ t[2][(c >> 16) & 0xFF] ^ t[3][c >> 24]
        c = np.where((behind >> np.uint64(k)) & np.uint64(1), moved, c).astype(np.uint32)
    return int(np.bitwise_xor.reduce(c)), int(l.sum(dtype=np.uint64))


def fold(checks, lens, wrap):
    """fold_scalar for short tables and for Adler-32; the vector form for long CRC tables (tests/test_emu_checksum_pack.py holds the
    two against each other)"""
    if wrap == 2 and len(lens) > 300:
        return fold_crc_vector(checks, lens)
    return fold_scalar(checks, lens, wrap)


def header_bytes(wrap, level, strategy):
    """what deflateInit2_(level, Z_DEFLATED, 15 / 31, 8, strategy) + deflate() write in front of the deflate data"""
    if wrap == 0:
        return b""
    co = zlib.compressobj(level, zlib.DEFLATED, 15 if wrap == 1 else 31, 8, strategy)
    out = co.compress(b"") + co.flush()
    return out[:2 if wrap == 1 else 10]


def trailer_bytes(wrap, check, raw_len):
    if wrap == 1:
        return struct.pack(">I", check)
    if wrap == 2:
        return struct.pack("<II", check, raw_len & 0xFFFFFFFF)
    return b""


# ---- 1. the checksum kernel ----------------------------------------------------------------------------------------------
# every threshold of zmi_checksum_kernel and its neighbours: the 16-byte stripe, the 4 KiB a workgroup takes per Adler trip, the
# first and second trip of the four-stripe loop for thread 0 (3 * 4096 + 16, + 16384) and for thread 255, the 16 KiB CRC block
CHECKSUM_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257,
                    4079, 4080, 4081, 4095, 4096, 4097,
                    12303, 12304, 12305,
                    16383, 16384, 16385,
                    16384 + 63, 16384 + 64, 16384 + 65,
                    28687, 28688, 28689,
                    32767, 32768, 32769, 3 * 16384 + 7, 65535, 65536, 65537, (1 << 20) + 1]
CHECKSUM_CONTENTS = ["ff", "zero", "first_ff", "last_ff", "mod251", "random"]
CHECKSUM_KINDS = [1, 2, 3]
GAP = 0xA5   # between the shards: a read outside a shard changes its sums
_LONG = {}


def _content(name, n):
    if name == "ff":
        return np.full(n, 0xFF, dtype=np.uint8)
    if name in ("zero", "first_ff", "last_ff"):
        a = np.zeros(n, dtype=np.uint8)
        if n and name == "first_ff":
            a[0] = 0xFF
        if n and name == "last_ff":
            a[-1] = 0xFF
        return a
    if name not in _LONG:
        m = (1 << 20) + 1
        _LONG[name] = (np.arange(m, dtype=np.uint32) % 251).astype(np.uint8) if name == "mod251" else \
            np.random.default_rng(20240517).integers(0, 256, m, dtype=np.uint8)
    return _LONG[name][:n]


def _layout(lengths, residues, start=0):
    """back-to-back shards, each moved up to the next address with the residue asked for, at least one byte apart"""
    off, pos = [], start
    for n, r in zip(lengths, residues):
        pos += (r - pos) % 16
        off.append(pos)
        pos += n + 1
    return np.array(off, dtype=np.uint64), pos + 16


def _init_words(n, salt):
    return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(salt)) | np.uint32(1)


def _check_launch(tag, addr, off, lens, kind, init, got, want_adler, want_crc, residues=None):
    a0, c0 = init
    a, c = got
    if residues is not None:
        assert [(addr + int(o)) % 16 for o in off] == list(residues), tag   # the residue of the ADDRESS the kernel sees
    for i in range(len(lens)):
        where = (tag, "shard", i, "len", int(lens[i]), "residue", (addr + int(off[i])) % 16, "kind", kind)
        if kind & 1:
            assert int(a[i]) == want_adler[i], where + ("adler", hex(int(a[i])), hex(want_adler[i]))
        else:
            assert int(a[i]) == int(a0[i]), where + ("adler array written",)
        if kind & 2:
            assert int(c[i]) == want_crc[i], where + ("crc", hex(int(c[i])), hex(want_crc[i]))
        else:
            assert int(c[i]) == int(c0[i]), where + ("crc array written",)


def checksum_matrix(target, content, lengths=CHECKSUM_LENGTHS, kinds=CHECKSUM_KINDS):
    """every length x every start residue 0..15 with one kind of contents, one buffer, one launch per kind; the array that was not
    asked for keeps its values.  Returns the number of (length, residue, kind) cases."""
    ls = [n for n in lengths for _ in range(16)]
    rs = [r for _ in lengths for r in range(16)]
    off, size = _layout(ls, rs)
    buf = np.full(size, GAP, dtype=np.uint8)
    ref = {}
    for o, n in zip(off, ls):
        d = _content(content, n)
        buf[int(o):int(o) + n] = d
        if n not in ref:
            ref[n] = (zlib.adler32(d.tobytes()), zlib.crc32(d.tobytes()))
    lens = np.array(ls, dtype=np.uint32)
    launches = [(off, lens, k, _init_words(len(ls), 11 * k), _init_words(len(ls), 13 * k + 5)) for k in kinds]
    addr, res = target.checksums(buf, launches)
    for (o, l, k, a0, c0), got in zip(launches, res):
        _check_launch(content, addr, o, l, k, (a0, c0), got, [ref[n][0] for n in ls], [ref[n][1] for n in ls], rs)
    return len(ls) * len(kinds)


def checksum_fixed_launches(target):
    """a launch of one shard, and one of 3500 short ragged shards with empty ones among them"""
    rng = np.random.default_rng(99)
    ls = [int(x) for x in rng.integers(0, 300, 3500)]
    for i in range(0, 3500, 9):
        ls[i] = 0
    rs = [int(x) for x in rng.integers(0, 16, 3500)]
    off, size = _layout(ls, rs, start=2048)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    one_off, one_len = np.array([5], dtype=np.uint64), np.array([1000], dtype=np.uint32)
    lens = np.array(ls, dtype=np.uint32)
    launches = [(one_off, one_len, 3, _init_words(1, 1), _init_words(1, 2)), (off, lens, 3, _init_words(3500, 3), _init_words(3500, 4))]
    addr, res = target.checksums(buf, launches)
    raw = buf.tobytes()
    for (o, l, k, a0, c0), got, tag in zip(launches, res, ("one shard", "3500 shards")):
        pieces = [raw[int(x):int(x) + int(n)] for x, n in zip(o, l)]
        _check_launch(tag, addr, o, l, k, (a0, c0), got, [zlib.adler32(p) for p in pieces], [zlib.crc32(p) for p in pieces])
    assert ls.count(0) >= 300
    return 3501


def checksum_large_ff(target, n=(64 << 20) + 5):
    """the largest sums there are: one shard of n bytes 0xFF, at a 16-byte aligned address (four-stripe loop, CRC blocks) and at
    residue 3 (byte-wise loads, per-thread segments)"""
    buf = np.full(n + 16, 0xFF, dtype=np.uint8)
    want = (zlib.adler32(buf[:n].tobytes()), zlib.crc32(buf[:n].tobytes()))
    lens = np.array([n], dtype=np.uint32)
    launches = [(np.array([r], dtype=np.uint64), lens, 3, _init_words(1, r), _init_words(1, r + 1)) for r in (0, 3)]
    addr, res = target.checksums(buf, launches)
    for (o, l, k, a0, c0), got, r in zip(launches, res, (0, 3)):
        _check_launch("0xFF x %d" % n, addr, o, l, k, (a0, c0), got, [want[0]], [want[1]], [r])
    return 2


# ---- 2. the combine kernel -----------------------------------------------------------------------------------------------
COMBINE_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 300, 4095, 4096, 4097, 8193, 70000]
COMBINE_WORLDS = [1, 2, 3, 8]
COMBINE_PATTERNS = ["zero", "first", "last", "pow2", "max", "adler_edges", "random"]


def _combine_lens(pattern, n, rng):
    l = np.zeros(n, dtype=np.uint32)
    if n == 0 or pattern == "zero":
        return l
    if pattern == "first":
        l[0] = 123457
    elif pattern == "last":
        l[-1] = 0x80000001
    elif pattern == "pow2":
        l[:] = np.uint32(1) << (np.arange(n, dtype=np.uint32) % np.uint32(32))
    elif pattern == "max":
        l[:] = 0xFFFFFFFF
    elif pattern == "adler_edges":
        l[:] = np.array([65520, 65521, 65522, 2 * 65521, 3 * 65521, 65521 * 65537, 1, 7 * 65521 + 65520], dtype=np.uint32)[np.arange(n) % 8]
    else:
        l[:] = rng.integers(0, 1 << 21, n, dtype=np.uint32)
        l[rng.random(n) < 0.05] = 0
    return l


def _combine_checks(n, wrap):
    """a different value in every entry (a permutation or ordering error cannot cancel); Adler-32 halves below 65521, with 0 and
    65520 among them"""
    g = np.arange(n, dtype=np.uint64)
    if wrap == 2:
        return ((g * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (g * np.uint64(40503) + np.uint64(65520) + g // np.uint64(BASE)) % np.uint64(BASE)
    lo = (g * np.uint64(30011)) % np.uint64(BASE)
    c = ((hi << np.uint64(16)) | lo).astype(np.uint32)
    if n > 1:
        c[1] = 65520          # s2 = 0, s1 = 65520
    return c


def combine_table(n_entries, world, wrap, pattern, rng):
    """-> (checks, lens) as the rank-major table of world x ceil(n_entries / world) entries, (check, total) expected.  The short
    ranks are padded with entries of length 0 whose check field holds anything."""
    n_local = -(-n_entries // world)
    lens = np.zeros(world * n_local, dtype=np.uint32)
    checks = rng.integers(0, 1 << 32, world * n_local, dtype=np.uint64).astype(np.uint32)   # (what the padding keeps)
    lens[:n_entries] = _combine_lens(pattern, n_entries, rng)
    keep = lens != 0
    checks[keep] = _combine_checks(world * n_local, wrap)[keep]
    assert len(set(checks[keep].tolist())) == int(keep.sum())
    want = fold(checks, lens, wrap)
    idx = logical_order(world, n_local)
    t_checks, t_lens = np.zeros_like(checks), np.zeros_like(lens)
    t_checks[idx] = checks
    t_lens[idx] = lens
    return t_checks, t_lens, want


def combine_matrix(target, wrap, world, counts=COMBINE_COUNTS, patterns=COMBINE_PATTERNS):
    rng = np.random.default_rng(1000 * wrap + world)
    cases, above = 0, 0
    for n in counts:
        for pattern in patterns:
            if n == 0 and pattern != "zero":
                continue
            checks, lens, want = combine_table(n, world, wrap, pattern, rng)
            got = target.combine(checks, lens, wrap, world)
            assert got == want, (wrap, world, n, pattern, [hex(x) for x in got], [hex(x) for x in want])
            above += want[1] > 1 << 32
            cases += 1
    assert above >= 5   # 64-bit totals
    return cases


def combine_end_to_end(target, world):
    """checksums of ragged pieces of one buffer, laid out rank-major, combined: the check values of the whole buffer"""
    rng = np.random.default_rng(5 + world)
    sizes = [0, 1, 65521, (1 << 20) + 3, 0, 17, 4096, 65520, 3, 16385, 100000, 0, 255, 65522, 31]
    total = sum(sizes)
    buf = rng.integers(0, 256, total + 16, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    lens = np.array(sizes, dtype=np.uint32)
    n = len(sizes)
    _, res = target.checksums(buf, [(off, lens, 3, np.zeros(n, np.uint32), np.zeros(n, np.uint32))])
    adler, crc = res[0]
    n_local = -(-n // world)
    idx = logical_order(world, n_local)[:n]
    whole = buf[:total].tobytes()
    for wrap, per_piece, want in ((1, adler, zlib.adler32(whole)), (2, crc, zlib.crc32(whole))):
        t_checks = np.full(world * n_local, 0xDEADBEEF, dtype=np.uint32)
        t_lens = np.zeros(world * n_local, dtype=np.uint32)
        t_checks[idx] = per_piece
        t_lens[idx] = lens
        assert target.combine(t_checks, t_lens, wrap, world) == (want, total), (wrap, world)
    return 2


# ---- 3. scan and stitch plan ---------------------------------------------------------------------------------------------
SCAN_COUNTS = [0, 1, 2, 1023, 1024, 1025, 2049, 100000]


def _sizes(n, rng):
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s[rng.random(n) < 0.1] = 0
    s[rng.random(n) < 0.1] = 0xFFFFFFFF
    if n:
        s[0] = 0xFFFFFFFF
        s[-1] = 0 if n > 1 else 0xFFFFFFFF
    return s


def scan_checks(target, counts=SCAN_COUNTS):
    rng = np.random.default_rng(3)
    above = 0
    for n in counts:
        for sizes in (_sizes(n, rng), np.full(n, 0xFFFFFFFF, dtype=np.uint32), (rng.integers(0, 70000, n)).astype(np.uint32)):
            want = np.concatenate([[0], np.cumsum(sizes.astype(np.uint64), dtype=np.uint64)]).astype(np.uint64)
            got = target.scan_sizes(sizes)
            assert got.shape == want.shape and np.array_equal(got, want), (n, int(np.argmax(got != want)))
            above += int(want[-1]) > 1 << 32
    assert above >= 10
    return 3 * len(counts)


def stitch_plan_checks(target, worlds=(1, 2, 3, 8), n_locals=(1, 5, 1024, 1025)):
    rng = np.random.default_rng(4)
    for world in worlds:
        for n_local in n_locals:
            table = _sizes(world * n_local, rng).reshape(world, n_local)
            idx = logical_order(world, n_local)
            flat = table.reshape(-1).astype(np.uint64)
            g_off = np.cumsum(flat[idx], dtype=np.uint64) - flat[idx]          # exclusive, in logical order
            want_goff = np.zeros(world * n_local, dtype=np.uint64)
            want_goff[idx] = g_off
            rows = np.cumsum(table.astype(np.uint64), axis=1, dtype=np.uint64)
            want_soff = np.concatenate([np.zeros((world, 1), dtype=np.uint64), rows], axis=1)
            want_tot = [int(x) for x in rows[:, -1]] + [int(flat.sum(dtype=np.uint64))]
            goff, soff, totals = target.stitch_plan(table)
            assert np.array_equal(goff.reshape(-1), want_goff), (world, n_local)
            assert np.array_equal(soff, want_soff), (world, n_local)
            assert list(totals) == want_tot, (world, n_local)
    return len(worlds) * len(n_locals)


# ---- 4. the copy kernel --------------------------------------------------------------------------------------------------
COPY_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 4079, 4080, 4081, 4095, 4096, 4097, 4111, 4112, 8191, 8192, 8193, 3 * 4096 + 5]
COPY_LARGE = (1 << 20) + 3
SENTINEL = 0xC3


def _copy_case(target, tag, ranges, max_len=None, dst_cap=None, expect_split=None):
    """ranges: [(length, source residue, destination residue)].  Source and destination ranges lie apart by at least a byte, the
    destination starts as SENTINEL everywhere: afterwards it equals the sentinel array with the source bytes sliced in."""
    ls = [r[0] for r in ranges]
    soff, ssize = _layout(ls, [r[1] for r in ranges], start=3)
    doff, dsize = _layout(ls, [r[2] for r in ranges], start=7)
    src = np.random.default_rng(len(ranges)).integers(0, 256, ssize, dtype=np.uint8)
    dst = np.full(dsize, SENTINEL, dtype=np.uint8)
    lens = np.array(ls, dtype=np.uint32)
    cap = dsize if dst_cap is None else dst_cap
    mx = max(ls) if max_len is None else max_len
    if expect_split is not None:   # the rule of zmi_launch_copy_ranges, so that the case is the geometry it is meant to be
        split, tiles = 1, (mx + 4095) // 4096
        while len(ls) * split < 4096 and split < tiles:
            split *= 2
        assert (split > 1) == expect_split, (tag, split)
    want = dst.copy()
    skipped = 0
    for o, d, n in zip(soff, doff, ls):
        if int(d) + n > cap:
            skipped += 1
            continue
        want[int(d):int(d) + n] = src[int(o):int(o) + n]
    sa, da, got = target.copy_ranges(src, soff, 0, lens, mx, dst, doff, cap)
    assert [(sa + int(o)) % 16 for o in soff] == [r[1] for r in ranges], tag
    assert [(da + int(d)) % 16 for d in doff] == [r[2] for r in ranges], tag
    if not np.array_equal(got, want):
        bad = int(np.argmax(got != want))
        k = int(np.searchsorted(doff, bad, side="right")) - 1
        raise AssertionError((tag, "first wrong byte", bad, "range", k, ranges[max(k, 0)], "at", bad - int(doff[max(k, 0)])))
    return len(ranges), skipped


def copy_many_ranges(target, lengths=COPY_LENGTHS):
    """every length x source residue x destination residue in one launch of more than 4096 ranges (one workgroup per range)"""
    ranges = [(n, s, d) for n in lengths for s in range(16) for d in range(16)]
    assert len(ranges) >= 4096
    return _copy_case(target, "many", ranges, expect_split=False)[0]


def copy_few_large_ranges(target, large=COPY_LARGE):
    """launches of a few ranges, several workgroups per range: sixteen of 1 MiB + 3 with every source and every destination residue,
    and the multi-tile lengths of the list above"""
    n = _copy_case(target, "large", [(large, s, (5 * s + 3) % 16) for s in range(16)], expect_split=True)[0]
    few = [(l, (3 * i + 1) % 16, (7 * i + 2) % 16) for i, l in enumerate([8191, 8192, 8193, 3 * 4096 + 5, 4097, 0, 1, 4112, 3 * 4096 + 5, 8193, 33])]
    n += _copy_case(target, "few", few, expect_split=True)[0]
    # a max_len below the longest range only changes the split, never the bytes
    n += _copy_case(target, "few, short max_len", few, max_len=4097, expect_split=True)[0]
    return n


def copy_capacity(target):
    """a range that ends behind dst_cap is skipped whole -- its bytes below the capacity keep the sentinel too -- the others are copied"""
    ranges = [(5000, 1, 2), (4096, 0, 0), (33, 5, 9), (9000, 7, 3), (100, 2, 4)]
    ls = [r[0] for r in ranges]
    doff, dsize = _layout(ls, [r[2] for r in ranges], start=7)
    n = 0
    for cap in (int(doff[3]) + 9000 - 1, int(doff[3]) + 9000, int(doff[2]) + 33, int(doff[2]) + 32, int(doff[1]) + 10):
        cases, skipped = _copy_case(target, "cap %d" % cap, ranges, dst_cap=cap)
        assert skipped == sum(int(d) + l > cap for d, l in zip(doff, ls))
        n += cases
    return n


def pack_slab_checks(target):
    """the slot form (source offset = index * stride, destinations dense from the scan): odd strides give every source residue"""
    n = 0
    for stride, count in ((4129, 320), (12301, 40)):
        rng = np.random.default_rng(stride)
        ls = [COPY_LENGTHS[i % len(COPY_LENGTHS)] for i in range(count)]
        ls = [l if l <= stride else stride for l in ls]
        slots = rng.integers(0, 256, (count, stride), dtype=np.uint8)
        total = sum(ls)
        slab = np.full(total + 16, SENTINEL, dtype=np.uint8)
        lens = np.array(ls, dtype=np.uint32)
        addr, got, off = target.pack_slab(slots, lens, slab)
        assert addr % 16 == 0 and len({(i * stride) % 16 for i in range(count)}) == 16
        want_off = np.concatenate([[0], np.cumsum(ls)]).astype(np.uint64)
        assert np.array_equal(off, want_off), stride
        want = np.concatenate([slots[i, :l] for i, l in enumerate(ls)] + [np.full(16, SENTINEL, dtype=np.uint8)])
        assert np.array_equal(got, want), (stride, int(np.argmax(got != want)))
        n += count
    return n


# ---- 5. the frame kernel -------------------------------------------------------------------------------------------------
FRAME_PAYLOADS = [0, 1, 4097]
FRAME_RAW = [5, (1 << 32) - 1, (1 << 32) + 5]
FRAME_CHECKS = [0, 0x01020304, 0xFFFFFFFF]


def _frame_case(target, wrap, level, strategy, payload, raw_len, check):
    head, tail = header_bytes(wrap, level, strategy), trailer_bytes(wrap, check, raw_len)
    total = len(head) + payload + len(tail)
    room = total + 32
    filled = ((np.arange(room, dtype=np.uint32) * 7 + 3) % 251).astype(np.uint8)
    where = (wrap, level, strategy, payload, raw_len, hex(check))
    # enough room, and exactly enough
    for cap in (room - 5, total):
        out, length, status = target.frame(filled.copy(), cap, payload, check, raw_len, wrap, level, strategy)
        assert status == 0 and length == total, where + (cap, status, length)
        assert out[:len(head)].tobytes() == head, where + (out[:len(head)].tobytes().hex(), head.hex())
        assert np.array_equal(out[len(head):len(head) + payload], filled[len(head):len(head) + payload]), where
        assert out[len(head) + payload:total].tobytes() == tail, where + (out[len(head) + payload:total].tobytes().hex(), tail.hex())
        assert np.array_equal(out[total:], filled[total:]), where      # the guard bytes
    n = 2
    if total:   # one byte short: Z_BUF_ERROR, the length it needs, no trailer
        out, length, status = target.frame(filled.copy(), total - 1, payload, check, raw_len, wrap, level, strategy)
        assert status == -5 and length == total, where + (status, length)
        assert np.array_equal(out[len(head):], filled[len(head):]), where
        n += 1
    return n


def frame_checks(target, wrap):
    """every level and strategy (the header's FLEVEL / XFL), the payload lengths, raw lengths and check values taken in turn so
    that each combination of the three occurs; at level 6 and 9 with the default strategy all of them"""
    trio = [(p, r, c) for p in FRAME_PAYLOADS for r in FRAME_RAW for c in FRAME_CHECKS]
    n, k = 0, 0
    for level in range(10):
        for strategy in range(5):
            for _ in range(2):
                n += _frame_case(target, wrap, level, strategy, *trio[k % len(trio)])
                k += 1
    assert k >= len(trio)
    for level in (6, 9):
        for p, r, c in trio:
            n += _frame_case(target, wrap, level, 0, p, r, c)
    return n
