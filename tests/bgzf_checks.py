"""Checks of the BGZF writer (zmi_bgzf_bound / zmi_bgzf_blocks_dev / zmi_bgzf_deflate_dev, include/zmi355.h), shared by
tests/test_emu_bgzf.py (CPU, the emulator build) and tests/test_gpu_bgzf.py (the MI355X), both through the C ABI on buffers a `mem`
object owns (put / full / read / stream, as in tests/ranges_checks.py).

The judges are Python's gzip.decompress for the whole file, zlib.decompressobj(-15) and zlib.crc32 per block, and the block walker
below, which compares every header byte, follows BSIZE + 1 from offset 0 and requires the chain to land exactly on the 28
end-of-file bytes at the end of the file.  The library's own readers never judge alone."""
import ctypes as C
import functools
import gzip
import random
import struct
import zlib

import numpy as np

BLOCK_MAX, HEADER, EOF_LEN = 65280, 18, 28
HEAD16 = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF = HEAD16 + bytes.fromhex("1b00" "0300" "0000000000000000")
Z_BUF_ERROR, E_ARG = -5, -103
GUARD, FILL = 64, 0xC7
CANARY = 0x7777777777777777

NS = [0, 1, 5, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 17]
BBS = [65280, 4096, 777, 1]
SHIFTS = [0, 1, 3, 15]
CONFIGS = [(0, 0), (1, 0), (6, 0), (9, 0), (6, 2), (6, 3)]     # (level, strategy): levels 0 / 1 / 6 / 9, strategies 0 / 2 / 3 at level 6
KINDS = ["text", "zeros", "random", "mix"]


def bind(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_deflate_bound.restype = u64
    L.zmi_deflate_bound.argtypes = [u64, i32]
    L.zmi_deflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, vp, u64, vp, vp, vp]
    L.zmi_bgzf_bound.restype = u64
    L.zmi_bgzf_bound.argtypes = [u64, u32]
    L.zmi_bgzf_blocks_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_bgzf_deflate_dev.argtypes = [vp, vp, u64, u32, i32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_gzip_find_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_inflate_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    return L


# ---- data -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _text(n, seed):
    r = random.Random(seed)
    words = [bytes(r.randrange(97, 123) for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + (b" " if r.random() < 0.9 else bytes([r.randrange(256)]))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def _noise(n, seed):
    return np.random.RandomState(seed).bytes(n)


@functools.lru_cache(maxsize=None)
def make(kind, n, block_bytes=BLOCK_MAX, seed=1):
    """text, zeros, random bytes, or ("mix") the three in turn, one per block"""
    if kind == "text":
        return _text(n, seed)
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return _noise(n, seed)
    parts = []
    for i, at in enumerate(range(0, n, block_bytes)):
        parts.append(make(KINDS[i % 3], min(block_bytes, n - at), block_bytes, seed + i))
    return b"".join(parts)


def reproducible(level, strategy):
    """May two calls be compared byte for byte?  At every level.  (Until a producer of the match search waited for BOTH chunks its tile
    reads, levels 1 and 3 -- three hash-building waves -- gave different, equally valid streams from call to call on the MI355X, and
    this returned False for them: DESIGN.md section 19, csrc/lz77.hip; tests/test_gpu_schedule.py holds the device to it.)"""
    return True


def kind_of_block(kind, i):
    return KINDS[i % 3] if kind == "mix" else kind


def cut(data, block_bytes):
    return [data[at:at + block_bytes] for at in range(0, len(data), block_bytes)]


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
def walk(file):
    """-> (offsets of every block and then of the end-of-file block, payloads, raw bytes per block)"""
    at, offs, payloads, raws = 0, [], [], []
    while True:
        assert at + EOF_LEN <= len(file), (at, len(file))
        assert file[at:at + 16] == HEAD16, (at, file[at:at + 16].hex())
        size = struct.unpack_from("<H", file, at + 16)[0] + 1
        assert size >= EOF_LEN and at + size <= len(file), (at, size, len(file))
        payload = file[at + HEADER:at + size - 8]
        crc, isize = struct.unpack_from("<II", file, at + size - 8)
        d = zlib.decompressobj(-15)
        raw = d.decompress(payload)
        assert d.eof and not d.unused_data, at              # a complete stream, BFINAL set, nothing behind it
        assert isize == len(raw) and crc == zlib.crc32(raw), at
        offs.append(at)
        if at + size == len(file):
            assert file[at:] == EOF                          # the chain lands exactly on the end-of-file block
            return offs, payloads, raws
        payloads.append(payload)
        raws.append(raw)
        at += size


def stored(raw):
    return b"\x01" + struct.pack("<HH", len(raw), len(raw) ^ 0xFFFF) + raw


def bound(n, block_bytes):
    return n + 31 * (-(-n // block_bytes)) + EOF_LEN


class Res:
    def __init__(self, rc, status=0, total=0, buf=b"", guard_ok=True, off=None, blen=None):
        self.rc, self.status, self.total, self.buf, self.guard_ok, self.off, self.blen = rc, status, total, buf, guard_ok, off, blen

    @property
    def file(self):
        return self.buf[:self.total]

    def __repr__(self):
        return "Res(rc=%d status=%d total=%d guard_ok=%s)" % (self.rc, self.status, self.total, self.guard_ok)


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem

    def _bytes(self, b, shift=0):
        return self.mem.put(np.frombuffer(bytes(b) + b"\0" * 16, dtype=np.uint8), shift)

    def deflate(self, data, block_bytes, level=6, strategy=0, shift=0, cap=None, index=True, null=None):
        """one zmi_bgzf_deflate_dev call; the index has one entry of canary behind the n_blocks + 1 the call owns"""
        m, n = self.mem, len(data)
        nb = -(-n // block_bytes) if 0 < block_bytes <= BLOCK_MAX else 0
        if cap is None:
            cap = int(self.L.zmi_bgzf_bound(n, block_bytes))
        inp, out = self._bytes(data, shift), m.full(cap + GUARD, FILL)
        olen, st, idx = m.full(8, 0x77), m.full(4, 0x77), m.put(np.full(nb + 2, CANARY, dtype=np.uint64))
        ptr = {"in": inp.ptr if n else None, "out": out.ptr, "len": olen.ptr, "st": st.ptr, "ctx": self.ctx}
        if null:
            ptr[null] = None
        rc = self.L.zmi_bgzf_deflate_dev(ptr["ctx"], ptr["in"], n, block_bytes, level, strategy, ptr["out"], cap, ptr["len"],
                                         idx.ptr if index else None, ptr["st"], m.stream)
        if rc != 0:
            return Res(rc)
        host, ix = m.read(out, np.uint8), m.read(idx, np.uint64)
        assert int(ix[nb + 1]) == CANARY and (index or int(ix[0]) == CANARY)
        return Res(0, int(m.read(st, np.int32)[0]), int(m.read(olen, np.uint64)[0]), host[:cap].tobytes(), bool((host[cap:] == FILL).all()),
                   [int(x) for x in ix[:nb + 1]] if index else None)

    def blocks(self, shards, max_len, level=6, strategy=0, cap=None, scattered=False, shift=0, want_len=True, null=None):
        """one zmi_bgzf_blocks_dev call.  scattered: the shards stand in reverse order with gaps of 3 bytes (any layout)"""
        m, n = self.mem, len(shards)
        offs, blob = [0] * n, bytearray()
        for i in (reversed(range(len(shards))) if scattered else range(len(shards))):
            offs[i] = len(blob)
            blob += shards[i] + (b"\xEE" * 3 if scattered else b"")
        if cap is None:
            cap = sum(len(s) + 31 for s in shards)
        inp, out = self._bytes(bytes(blob), shift), m.full(cap + GUARD, FILL)
        od, ld = m.put(np.array(offs + [0], dtype=np.uint64)), m.put(np.array([len(s) for s in shards] + [0], dtype=np.uint32))
        bo, bl, st = m.put(np.full(n + 2, CANARY, dtype=np.uint64)), m.put(np.full(n + 1, 0x77777777, dtype=np.uint32)), m.full(4, 0x77)
        ptr = {"in": inp.ptr, "off": od.ptr, "len": ld.ptr, "out": out.ptr, "boff": bo.ptr, "st": st.ptr, "ctx": self.ctx}
        if null:
            ptr[null] = None
        rc = self.L.zmi_bgzf_blocks_dev(ptr["ctx"], ptr["in"], ptr["off"], ptr["len"], n, max_len, level, strategy, ptr["out"], cap, ptr["boff"],
                                        bl.ptr if want_len else None, ptr["st"], m.stream)
        if rc != 0:
            return Res(rc)
        host, o, l = m.read(out, np.uint8), m.read(bo, np.uint64), m.read(bl, np.uint32)
        assert int(o[n + 1]) == CANARY and int(l[n]) == 0x77777777 and (want_len or n == 0 or int(l[0]) == 0x77777777)
        return Res(0, int(m.read(st, np.int32)[0]), int(o[n]), host[:cap].tobytes(), bool((host[cap:] == FILL).all()), [int(x) for x in o[:n + 1]],
                   [int(x) for x in l[:n]] if want_len else None)

    def raw_batch(self, shards, level=6, strategy=0):
        """what zmi_deflate_batch_dev(..., ZMI_WRAP_RAW) writes for every shard"""
        m, n = self.mem, len(shards)
        lens = [len(s) for s in shards]
        offs = [sum(lens[:i]) for i in range(n)]
        stride = int(self.L.zmi_deflate_bound(max(lens), 0))
        inp, out = self._bytes(b"".join(shards)), m.full(n * stride, 0)
        od, ld = m.put(np.array(offs, dtype=np.uint64)), m.put(np.array(lens, dtype=np.uint32))
        ol, st = m.full(4 * n, 0), m.full(4 * n, 0x77)
        rc = self.L.zmi_deflate_batch_dev(self.ctx, inp.ptr, od.ptr, ld.ptr, n, max(lens), level, strategy, 0, out.ptr, stride, ol.ptr, st.ptr, m.stream)
        assert rc == 0 and (m.read(st, np.int32)[:n] == 0).all()
        host, l = m.read(out, np.uint8), m.read(ol, np.uint32)
        return [host[i * stride:i * stride + int(l[i])].tobytes() for i in range(n)]

    def find(self, file):
        m, cap = self.mem, len(file) // 18 + 1
        inp, starts, cnt = self._bytes(file, 3), m.full(8 * cap, 0), m.full(4, 0x77)
        assert self.L.zmi_gzip_find_members_dev(self.ctx, inp.ptr, len(file), starts.ptr, cap, cnt.ptr, m.stream) == 0
        return [int(x) for x in m.read(starts, np.uint64)[:int(m.read(cnt, np.uint32)[0])]]

    def members(self, file, starts, out_cap):
        """-> (status, members, in_used, the output, member offsets) of one zmi_inflate_members_dev call"""
        m, k = self.mem, len(starts)
        inp, sd, out = self._bytes(file, 3), m.put(np.array(list(starts) + [0], dtype=np.uint64)), m.full(out_cap + GUARD, FILL)
        w, moff = m.full(32, 0x77), m.full(8 * (k + 1), 0)
        rc = self.L.zmi_inflate_members_dev(self.ctx, inp.ptr, len(file), sd.ptr, k, out.ptr, out_cap, w.ptr, w.ptr + 8, w.ptr + 16, moff.ptr,
                                            w.ptr + 20, w.ptr + 24, m.stream)
        assert rc == 0
        words = m.read(w, np.uint64)
        members, status = (int(x) for x in words[2:3].view(np.int32))
        host = m.read(out, np.uint8)
        assert (host[out_cap:] == FILL).all()
        return status, members, int(words[1]), host[:int(words[0])].tobytes(), [int(x) for x in m.read(moff, np.uint64)]


# ---- 1. shapes: every file is a BGZF file of the data, and the index is the walker's ---------------------------------------------------
def check_file(res, data, block_bytes, what=None):
    """the call's words and bytes against the judges -> (offsets, payloads)"""
    n = len(data)
    assert res.rc == 0 and res.status == 0 and res.guard_ok, (what, res)
    file = res.file
    assert res.total == len(file) <= bound(n, block_bytes), (what, res)
    assert gzip.decompress(file) == data, what
    offs, payloads, raws = walk(file)
    assert raws == cut(data, block_bytes), what                     # block i = [i * block_bytes, min(n, (i + 1) * block_bytes))
    assert offs[-1] == len(file) - EOF_LEN
    if res.off is not None:
        assert res.off == offs, what                                  # d_block_off: every block, then the end-of-file block
    for p, r in zip(payloads, raws):
        assert HEADER + len(p) + 8 <= len(r) + 31, what               # the 64 KiB limit is structural
    return offs, payloads


def shapes(target, configs=CONFIGS, kinds=KINDS, ns=NS, bbs=BBS, shifts=SHIFTS):
    done = 0
    for bb in bbs:
        for n in ns:
            if bb == 1 and n > 300:
                continue
            assert int(target.L.zmi_bgzf_bound(n, bb)) == bound(n, bb)
            for kind in kinds:
                data = make(kind, n, bb)
                for level, strategy in configs:
                    first = None
                    for shift in shifts:
                        res = target.deflate(data, bb, level, strategy, shift)
                        check_file(res, data, bb, (n, bb, kind, level, strategy, shift))
                        first = first or res.file
                        if reproducible(level, strategy):
                            assert res.file == first                  # the bytes do not depend on the alignment of the input
                        done += 1
    return done


# ---- 2. limit and fallback -------------------------------------------------------------------------------------------------------------
def fallback(target, configs=CONFIGS, bbs=(65280, 4096), blocks=6):
    """every payload is the batch encoder's raw stream of the shard, or, where that is longer than len + 5, one stored block (compared
    where two encoder calls give the same bytes, see reproducible()); at level 6 random blocks are stored, text and zero blocks the
    encoder's"""
    done = 0
    for bb in bbs:
        data = make("mix", blocks * bb - 1000, bb)
        shards = cut(data, bb)
        for level, strategy in configs:
            res = target.deflate(data, bb, level, strategy, 1)
            offs, payloads = check_file(res, data, bb)
            enc = target.raw_batch(shards, level, strategy) if reproducible(level, strategy) else payloads
            for i, (p, s, e) in enumerate(zip(payloads, shards, enc)):
                assert p == (e if len(e) <= len(s) + 5 else stored(s)), (bb, level, strategy, i)
                if (level, strategy) == (6, 0):
                    if kind_of_block("mix", i) == "random":
                        assert p == stored(s), (bb, i)                 # (the encoder's own answer where it is a single stored block)
                    else:
                        assert p == e != stored(s), (bb, i)
                done += 1
    return done


# ---- 3. the index is optional ------------------------------------------------------------------------------------------------------------
def index_optional(target):
    data = make("mix", 5 * 4096 + 9, 4096)
    a, b = target.deflate(data, 4096), target.deflate(data, 4096, index=False)
    check_file(a, data, 4096)
    assert b.rc == 0 and b.status == 0 and b.file == a.file and b.off is None
    return 2


# ---- 4. grouping -------------------------------------------------------------------------------------------------------------------------
def grouping(target, setenv, bb=4096, count=10):
    """the launch grouping, the call (whole buffer / batch, one batch / two), the layout and max_len do not change a byte"""
    data = make("mix", count * bb, bb)
    shards = cut(data, bb)
    one = target.deflate(data, bb)
    offs, _ = check_file(one, data, bb)
    done = 1
    try:
        for g in ("3", "7"):
            setenv("ZMI_STREAM_GROUP", g)
            r = target.deflate(data, bb)
            assert (r.rc, r.status, r.total, r.off) == (0, 0, one.total, one.off) and r.file == one.file, g
            s = target.blocks(shards, bb)
            assert s.rc == 0 and s.status == 0 and s.file + EOF == one.file and s.off == offs, g
            done += 2
    finally:
        setenv("ZMI_STREAM_GROUP", None)
    slab = target.blocks(shards, bb)
    assert slab.rc == 0 and slab.status == 0 and slab.guard_ok
    assert slab.file + EOF == one.file and slab.off == offs and slab.total == offs[-1]
    assert slab.blen == [b - a for a, b in zip(slab.off, slab.off[1:])]           # the table zmi_exchange_sizes takes
    for kw in ({"max_len": BLOCK_MAX}, {"max_len": bb, "scattered": True, "shift": 5}, {"max_len": bb, "want_len": False}):
        r = target.blocks(shards, **kw)
        assert (r.rc, r.status, r.off) == (0, 0, slab.off) and r.file == slab.file and r.guard_ok, kw
        done += 1
    a, b = target.blocks(shards[:4], bb), target.blocks(shards[4:], bb)           # two ranks' slabs
    assert a.status == 0 and b.status == 0 and a.file + b.file == slab.file
    assert a.blen + b.blen == slab.blen
    return done + 2


def empty_shards(target):
    """empty shards are legal: 28-byte blocks; no blocks at all: offset 0, status 0"""
    shards = [b"", _text(100, 3), b"", b"", _noise(2000, 4), b""]
    r = target.blocks(shards, 2000)
    assert r.rc == 0 and r.status == 0 and r.guard_ok, r
    offs, payloads, raws = walk(r.file + EOF)
    assert raws == shards and offs == r.off and r.blen[0] == r.blen[2] == r.blen[5] == EOF_LEN
    assert r.file[:EOF_LEN] == EOF and r.file[-EOF_LEN:] == EOF and payloads[4] == stored(shards[4])
    z = target.blocks([], 100)
    assert (z.rc, z.status, z.total, z.off, z.guard_ok) == (0, 0, 0, [0], True), z
    z = target.blocks([b"", b""], 0)
    assert (z.rc, z.status, z.file) == (0, 0, EOF + EOF), z
    e = target.deflate(b"", BLOCK_MAX)
    assert (e.rc, e.status, e.file, e.off) == (0, 0, EOF, [0]), e                  # as bgzip writes for empty input
    return 4


# ---- 5. capacity -------------------------------------------------------------------------------------------------------------------------
def capacity(target, bb=4096):
    data = make("mix", 6 * bb + 123, bb)
    shards = cut(data, bb)
    full = target.deflate(data, bb)
    offs, _ = check_file(full, data, bb)
    total, blocks_end = full.total, offs[-1]
    mid = offs[3] + (offs[4] - offs[3]) // 2
    done = 0
    for cap in (total - 1, mid, total - 10, 0):            # one byte short, inside block 3, inside the end-of-file block, none
        r = target.deflate(data, bb, cap=cap)
        assert (r.rc, r.status, r.total) == (0, Z_BUF_ERROR, total) and r.guard_ok, (cap, r)
        assert r.off == offs, cap                            # exact whether or not the blocks fitted
        fit = max(o for o in offs if o <= cap)               # the blocks that end at or before cap are right, nothing else is written
        assert r.buf[:fit] == full.file[:fit] and r.buf[fit:] == bytes([FILL]) * (cap - fit), cap
        done += 1
    for cap in (blocks_end - 1, mid, 0):
        r = target.blocks(shards, bb, cap=cap)
        assert (r.rc, r.status, r.total) == (0, Z_BUF_ERROR, blocks_end) and r.guard_ok, (cap, r)
        assert r.off == offs and r.blen == [b - a for a, b in zip(offs, offs[1:])], cap
        fit = max(o for o in offs if o <= cap)
        assert r.buf[:fit] == full.file[:fit] and r.buf[fit:] == bytes([FILL]) * (cap - fit), cap
        done += 1
    for r in (target.deflate(data, bb, cap=total), target.blocks(shards, bb, cap=blocks_end)):      # exactly enough
        assert r.rc == 0 and r.status == 0 and r.guard_ok and r.buf == full.file[:len(r.buf)]
        done += 1
    return done


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------------------
def arguments(target):
    data = _text(5000, 9)
    shards = cut(data, 1000)
    bad = [target.deflate(data, 0), target.deflate(data, BLOCK_MAX + 1), target.blocks(shards, BLOCK_MAX + 1),
           target.deflate(data, 1000, level=10), target.deflate(data, 1000, level=-2), target.deflate(data, 1000, strategy=5),
           target.deflate(data, 1000, strategy=-1), target.blocks(shards, 1000, level=10), target.blocks(shards, 1000, strategy=5)]
    bad += [target.deflate(data, 1000, null=k) for k in ("ctx", "in", "out", "len", "st")]
    bad += [target.blocks(shards, 1000, null=k) for k in ("ctx", "in", "off", "len", "out", "boff", "st")]
    for i, r in enumerate(bad):
        assert r.rc == E_ARG, (i, r)
    assert int(target.L.zmi_bgzf_bound(12345, 0)) == 0
    # a shard longer than max_len: the table lives on the device, so ZMI_E_ARG arrives in the status word
    r = target.blocks(shards, 999)
    assert (r.rc, r.status) == (0, E_ARG) and r.guard_ok, r
    r = target.blocks(shards[:2] + [data[:1001]] + shards[2:], 1000)
    assert (r.rc, r.status) == (0, E_ARG) and r.guard_ok, r
    # level -1 is level 6
    assert target.deflate(data, 1000, level=-1).file == target.deflate(data, 1000, level=6).file
    return len(bad) + 3


# ---- 7. the library's own readers --------------------------------------------------------------------------------------------------------
def own_readers(target, bb=4096, n=5 * 4096 + 77):
    data = make("text", n, bb)
    res = target.deflate(data, bb)
    offs, _ = check_file(res, data, bb)
    assert target.find(res.file) == offs                                           # the proposals are exactly the index
    nb = len(offs) - 1
    status, members, used, out, moff = target.members(res.file, offs, n + 100)
    assert (status, members, used, out) == (0, nb + 1, len(res.file), data)         # (the end-of-file block is an empty member)
    assert moff[:nb] == [i * bb for i in range(nb)] and moff[nb:nb + 2] == [n, n]
    mix = make("mix", n, bb)                                                       # stored blocks read back too
    res = target.deflate(mix, bb)
    offs, _ = check_file(res, mix, bb)
    status, members, used, out, moff = target.members(res.file, offs, n)
    assert (status, members, used, out) == (0, nb + 1, len(res.file), mix)
    return 2
