"""Checks of the calls that inflate a batch without an output size table (zmi_inflate_sizes_dev / zmi_inflate_batch_packed_dev,
include/zmi355.h), shared by tests/test_emu_inflate_sizes.py (CPU, the emulator build through ctypes) and
tests/test_gpu_inflate_sizes.py (the MI355X through Engine).

The judge of sizes and bytes is Python's zlib on the CPU.  The judge of the words of failing streams is the library's own
zmi_inflate_batch_dev_ex given ample room, which tests/parity_checks.py pins on the reference's vectors.

A target offers (streams: list of bytes; every call places stream i `shifts[i]` bytes behind a 16-byte boundary)
    sizes(streams, wrap, hist=0, limit=0, shifts=None)              -> [Word(size, status, in_used, detail)]
    batch(streams, wrap, caps, zdict=None, align=1, set_limit=True) -> Decoded: zmi_inflate_batch_dev_ex (zdict: the shared-dictionary
                                                                       call) with out_off = the aligned scan of caps, under an
                                                                       inflate-out limit set for these caps (set_limit=False: under
                                                                       the context's limit as set_out_limit(nbytes) left it)
    packed(streams, wrap, out_cap, align=1, zdict=None, limit=0)    -> Decoded of ONE zmi_inflate_batch_packed_dev call
    rc_sizes(wrap=1, hist=0, null_ctx=False, n=1), rc_packed(wrap=1, align=1, zdict=None, null_ctx=False, n=1)  -> the return code
    own(shards, level, wrap)                                        -> what the library's deflate makes of the shards
"""
import functools
import json
import os
import random
import struct
import zlib

import deflate_craft
from members_checks import text

RAW, ZLIB, GZIP, AUTO = 0, 1, 2, 3
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
Z_NEED_DICT, Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR, E_ARG = 2, -3, -4, -5, -103
GUARD = 256
FILL = 0xC7
AMPLE = 2 << 20
HERE = os.path.dirname(os.path.abspath(__file__))

LENS = [0, 1, 2, 257, 258, 259, 4095, 4096, 4097, 65535, 65536, 65537, 300000, (1 << 20) + 1]
SMALL_LENS = [n for n in LENS if n < 300000]          # (the emulator's subset of the length x mode matrix)
MODES = [("l0", 0, 0), ("l1", 1, 0), ("l6", 6, 0), ("l9", 9, 0), ("fixed", 6, zlib.Z_FIXED), ("huff", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]
# prefixes of text(40000, 77) whose raw deflate stream (level 6) is 4095 / 4096 / 4097 and 7167 / 7168 / 7169 bytes long: the fast pass
# starts only with >= 4 KiB of input ahead and stages 3.5 KiB, the edges where the last pass hands over to the token rounds
EDGE_LENS = {4095: 10788, 4096: 10790, 4097: 10791, 7167: 19657, 7168: 19662, 7169: 19664}


class Word:
    def __init__(self, size, status, in_used, detail):
        self.size, self.status, self.in_used, self.detail = size, status, in_used, detail

    def key(self):
        return (self.size, self.status, self.in_used, self.detail)

    def __repr__(self):
        return "Word(size=%d status=%d in_used=%d detail=%d)" % self.key()


class Decoded:
    """rc; off: the n + 1 (packed) or n (batch) output offsets; words: Word per stream (size = d_out_len); out: the buffer up to
    out_cap; guard_ok: the GUARD bytes behind it still hold the fill"""
    def __init__(self, rc, off, words, out, guard_ok):
        self.rc, self.off, self.words, self.out, self.guard_ok = rc, off, words, out, guard_ok

    def piece(self, i):
        return self.out[self.off[i]:self.off[i] + self.words[i].size]


# ---- building streams -----------------------------------------------------------------------------------------------------------
def deflate(raw, wrap, level=6, strategy=0, zdict=None):
    kw = {"zdict": zdict} if zdict is not None else {}
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[GZIP if wrap == AUTO else wrap], 8, strategy, **kw)
    return c.compress(raw) + c.flush()


def inflate(stream, wrap, zdict=None):
    kw = {"zdict": zdict} if zdict is not None else {}
    d = zlib.decompressobj(47 if wrap == AUTO else WBITS[wrap], **kw)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def rand_bytes(n, seed):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""


@functools.lru_cache(maxsize=None)
def edge_payloads():
    """the six payloads of EDGE_LENS (searched again where this zlib cuts its blocks elsewhere)"""
    big = text(40000, 77)
    out = []
    for want, n in sorted(EDGE_LENS.items()):
        if len(deflate(big[:n], RAW)) != want:
            hits = [m for m in range(max(1, n - 3000), n + 3000) if len(deflate(big[:m], RAW)) == want]
            n = hits[0] if hits else n
        out.append(big[:n])
    return out


@functools.lru_cache(maxsize=None)
def payloads(lens=tuple(LENS)):
    """(name, payload, level, strategy) of the exactness batch: the same payloads in every mode, then the special ones"""
    ps = []
    base = text(max(lens), 1234)
    for name, level, strategy in MODES:
        for n in lens:
            ps.append(("%s/%d" % (name, n), base[:n], level, strategy))
    ps.append(("random in dynamic", rand_bytes(70000, 5), 6, 0))            # stored blocks inside a dynamic stream
    ps.append(("several stored", text(200000, 6), 0, 0))
    ps.append(("zeros", bytes(1 << 20), 6, 0))                              # chains of length-258 matches
    for p in edge_payloads():
        ps.append(("edge/%d" % len(p), p, 6, 0))
    return ps


@functools.lru_cache(maxsize=None)
def exact_batch(wrap, lens=tuple(LENS)):
    """(streams, payloads) of the exactness batch in one wrapper; auto alternates zlib and gzip streams"""
    streams, raws = [], []
    for i, (name, raw, level, strategy) in enumerate(payloads(lens)):
        w = (ZLIB, GZIP)[i & 1] if wrap == AUTO else wrap
        s = deflate(raw, w, level, strategy)
        assert inflate(s, wrap) == raw, name
        streams.append(s)
        raws.append(raw)
    assert 40 <= len(streams) < 512
    return streams, raws


def aligned_scan(sizes, align):
    off, at = [], 0
    for s in sizes:
        off.append(at)
        at += (s + align - 1) & ~(align - 1)
    return off + [at]


# ---- 1. sizes are exact -------------------------------------------------------------------------------------------------------------
def sizes_exact(target, wrap, lens=tuple(LENS)):
    streams, raws = exact_batch(wrap, lens)
    got = target.sizes(streams, wrap)
    for i, (w, s, r) in enumerate(zip(got, streams, raws)):
        assert w.key() == (len(r), 0, len(s), 0), (payloads(lens)[i][0], w, len(r), len(s))
    return len(streams)


def sizes_many_tiny(target, n=600):
    """above 512 streams the product's own selection is the one-wave kernel"""
    raws = [text(i % 97, 3000 + i) for i in range(n)]
    streams = [deflate(r, ZLIB, (0, 1, 6, 9)[i & 3]) for i, r in enumerate(raws)]
    got = target.sizes(streams, ZLIB)
    assert [w.key() for w in got] == [(len(r), 0, len(s), 0) for r, s in zip(raws, streams)]
    return n


def sizes_own_output(target, lens=(0, 1, 4097, 70000, 300000)):
    done = 0
    for level in (1, 6, 9):
        for wrap in (RAW, ZLIB, GZIP):
            raws = [text(n, 4000 + n) for n in lens]
            streams = target.own(raws, level, wrap)
            for s, r in zip(streams, raws):
                assert inflate(s, wrap) == r
            got = target.sizes(streams, wrap)
            assert [w.key() for w in got] == [(len(r), 0, len(s), 0) for r, s in zip(raws, streams)], (level, wrap, got)
            done += len(streams)
    return done


# ---- 3. failing streams (before 2: the independence check permutes them too) --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def failing(wrap):
    """(name, stream) in one wrapper: cuts, damaged blocks, and the bitstreams of tests/golden/inflate_vectors.json for that wrapper"""
    out = []
    raw = text(20000, 21)
    w = ZLIB if wrap == AUTO else wrap
    good = deflate(raw, w, 6)
    head = {RAW: 0, ZLIB: 2, GZIP: 10}[w]
    tail = {RAW: 0, ZLIB: 4, GZIP: 8}[w]
    if head:
        out.append(("cut in the header", good[:head - 1]))
    out.append(("cut in the dynamic header", good[:head + 12]))
    out.append(("cut in a block", good[:len(good) // 2]))
    out.append(("cut one byte before the end of the data", good[:len(good) - tail - 1]))
    if tail:
        out.append(("cut in the trailer", good[:len(good) - 2]))
    if w == GZIP:
        out.append(("cut behind the CRC", good[:len(good) - 4]))
        out.append(("cut behind a wrong CRC", good[:len(good) - 5] + bytes([good[-5] ^ 1]) + good[-4:-2]))
    wrapd = lambda body, payload=b"": {RAW: body, ZLIB: b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(payload)),
                                        GZIP: b"\x1f\x8b\x08\x00\0\0\0\0\0\x03" + body + struct.pack("<II", zlib.crc32(payload), len(payload))}[w]
    out.append(("block type 3", wrapd(b"\x07" + bytes(8))))
    out.append(("stored block, wrong NLEN", wrapd(b"\x01\x05\x00\x00\x00hello")))
    out.append(("stored block, cut", wrapd(b"\x01\x05\x00\xfa\xffhel")[:8 + head]))
    out.append(("distance one byte in front of the start", wrapd(deflate_craft.fixed_block([97, 98, 99, (4, 4)]))))
    out.append(("good", good))
    if w == ZLIB:
        out.append(("FDICT", deflate(raw[:500], ZLIB, 6, zdict=b"a dictionary of some words")))
        out.append(("bad header check", b"\x78\x9d" + good[2:]))
    for v in json.load(open(os.path.join(HERE, "golden", "inflate_vectors.json")))["bitstreams"]:
        if v["wrap"] == wrap:
            out.append((v["source"].split(":")[-1], bytes.fromhex(v["input"])))
    return out


def _check_blind(judge, stream, wrap):
    """the one stated difference: where the judge's Z_DATA_ERROR is a check value's (zlib says which, and fed byte by byte, where), the
    size pass reports 0 for a full-length trailer and truncation for a gzip trailer that ends inside ISIZE"""
    if (judge.status, judge.detail) != (Z_DATA_ERROR, 0):
        return judge.key()
    d = zlib.decompressobj(47 if wrap == AUTO else WBITS[wrap])
    for i in range(len(stream)):
        try:
            d.decompress(stream[i:i + 1])
        except zlib.error as e:
            if "incorrect length check" in str(e):
                return (judge.size, 0, judge.in_used, 0)
            if "incorrect data check" in str(e):
                short = stream[:2] == b"\x1f\x8b" and len(stream) - (i + 1) < 4
                return (judge.size, Z_BUF_ERROR, judge.in_used, 1) if short else (judge.size, 0, judge.in_used, 0)
            break
    return judge.key()


def failing_streams(target, wrap):
    names, streams = zip(*failing(wrap))
    judge = target.batch(list(streams), wrap, [AMPLE] * len(streams))
    assert judge.rc == 0 and judge.guard_ok
    got = target.sizes(list(streams), wrap)
    bad = 0
    for name, s, w, j in zip(names, streams, got, judge.words):
        assert w.key() == _check_blind(j, s, wrap), (name, w, j)
        bad += w.status != 0
    assert bad >= 6
    by = dict(zip(names, got))
    assert (by["block type 3"].status, by["block type 3"].detail) == (Z_DATA_ERROR, 16 + 2)
    assert (by["stored block, wrong NLEN"].status, by["stored block, wrong NLEN"].detail) == (Z_DATA_ERROR, 16 + 1)
    assert (by["distance one byte in front of the start"].status, by["distance one byte in front of the start"].detail, by["distance one byte in front of the start"].size) == (Z_DATA_ERROR, 16 + 9, 3)
    assert by["cut in a block"].status == Z_BUF_ERROR and by["cut in a block"].detail == 1 and 0 < by["cut in a block"].size < 20000
    assert by["good"].key() == (20000, 0, len(streams[names.index("good")]), 0)
    if "FDICT" in by:
        assert by["FDICT"].status == Z_NEED_DICT
    return len(streams)


def history(target):
    """the stream whose match starts one byte in front of its output: a data error with no history, fine with 32 bytes of it"""
    s = deflate_craft.fixed_block([97, 98, 99, (4, 4)])
    fd = deflate(text(500, 3), ZLIB, 6, zdict=b"a dictionary of some words")
    assert target.sizes([s], RAW)[0].key() == (3, Z_DATA_ERROR, target.batch([s], RAW, [AMPLE]).words[0].in_used, 16 + 9)
    assert target.sizes([s], RAW, hist=32)[0].key() == (7, 0, len(s), 0)
    assert target.sizes([s], RAW, hist=1)[0].key() == (7, 0, len(s), 0)
    assert target.sizes([fd], ZLIB)[0].status == Z_NEED_DICT
    assert target.sizes([fd], ZLIB, hist=26)[0].key() == (500, 0, len(fd), 0)
    return 5


def wrong_checks(target):
    """a flipped CRC-32, Adler-32 and ISIZE: 0 and the right size from the size pass, -3 and the right bytes from the packed call"""
    raw = text(5000, 31)
    g, z = bytearray(deflate(raw, GZIP)), bytearray(deflate(raw, ZLIB))
    crc, isize, adler = bytearray(g), bytearray(g), bytearray(z)
    crc[-8] ^= 1
    isize[-4] ^= 1
    adler[-1] ^= 1
    for wrap, streams in ((GZIP, [bytes(crc), bytes(g), bytes(isize)]), (ZLIB, [bytes(adler), bytes(z)]), (AUTO, [bytes(crc), bytes(adler), bytes(isize)])):
        got = target.sizes(streams, wrap)
        assert [w.key() for w in got] == [(len(raw), 0, len(s), 0) for s in streams], (wrap, got)
        p = target.packed(streams, wrap, len(raw) * len(streams))
        assert p.rc == 0 and p.guard_ok and p.off == aligned_scan([len(raw)] * len(streams), 1)
        for i, s in enumerate(streams):
            good = s in (bytes(g), bytes(z))
            assert p.words[i].status == (0 if good else Z_DATA_ERROR) and p.words[i].size == len(raw) and p.piece(i) == raw, (wrap, i, p.words[i])
    return 3


# ---- 2. independence ----------------------------------------------------------------------------------------------------------------
def independence(target, wrap, lens=(0, 1, 259, 4097, 65537)):
    """the words of a stream do not depend on its place in the batch, on the batch, or on the alignment of its first byte"""
    base = text(max(lens), 1234)
    streams = [deflate(base[:n], ZLIB if wrap == AUTO else wrap, level) for n in lens for level in (0, 1, 6)]
    streams += [s for _, s in failing(wrap)][:8] + [deflate(p, GZIP if wrap == AUTO else wrap) for p in edge_payloads()[1:5:3]]
    want = [w.key() for w in target.sizes(streams, wrap, shifts=[0] * len(streams))]
    r = random.Random(8)
    for shift in (0, 1, 15):
        order = list(range(len(streams)))
        r.shuffle(order)
        got = target.sizes([streams[i] for i in order], wrap, shifts=[shift] * len(streams))
        assert [w.key() for w in got] == [want[i] for i in order], (wrap, shift)
    for i in range(0, len(streams), 3):
        for shift in (1, 15):
            assert target.sizes([streams[i]], wrap, shifts=[shift])[0].key() == want[i], (wrap, i, shift)
    return len(streams)


# ---- 4. size_limit ------------------------------------------------------------------------------------------------------------------
def size_limit(target):
    raws = [text(n, 50 + n) for n in (999, 1000, 1001)]
    done = 0
    for level in (0, 1, 6):                      # stored blocks, the fixed code, dynamic codes
        streams = [deflate(r, ZLIB, level) for r in raws]
        got = target.sizes(streams, ZLIB, limit=1000)
        assert got[0].key() == (999, 0, len(streams[0]), 0) and got[1].key() == (1000, 0, len(streams[1]), 0), got
        assert (got[2].size, got[2].status, got[2].detail) == (1000, Z_BUF_ERROR, 2), got
        assert [w.key() for w in target.sizes(streams, ZLIB)] == [(len(r), 0, len(s), 0) for r, s in zip(raws, streams)]
        p = target.packed(streams, ZLIB, 4096, limit=1000)
        assert p.rc == 0 and p.guard_ok and p.off == [0, 999, 1999, 2999], p.off
        assert p.piece(0) == raws[0] and p.piece(1) == raws[1]
        assert [(w.status, w.detail) for w in p.words] == [(0, 0), (0, 0), (Z_BUF_ERROR, 2)], p.words
        assert p.words[2].size <= 1000 and p.piece(2) == raws[2][:p.words[2].size]
        assert p.out[2999:] == bytes([FILL]) * (4096 - 2999)
        done += 1
    # a stream far above the limit, and one whose fast passes would run past it: the size is the limit, never a wrapped count
    big = [deflate(bytes(1 << 20), ZLIB), deflate(text(300000, 9), ZLIB)]
    for lim in (1, 65536, 299999):
        got = target.sizes(big, ZLIB, limit=lim)
        assert [(w.size, w.status, w.detail) for w in got] == [(lim, Z_BUF_ERROR, 2)] * 2, (lim, got)
    got = target.sizes(big, ZLIB, limit=300000)
    assert (got[0].size, got[0].status) == (300000, Z_BUF_ERROR) and got[1].key() == (300000, 0, len(big[1]), 0)
    return done + 4


# ---- 5. packed equals batch ----------------------------------------------------------------------------------------------------------
def _same_as_batch(target, streams, wrap, sizes, align, zdict=None, raws=None):
    off = aligned_scan(sizes, align)
    ref = target.batch(streams, wrap, sizes, zdict=zdict, align=align)
    p = target.packed(streams, wrap, off[-1], align=align, zdict=zdict)
    assert ref.rc == 0 and p.rc == 0 and ref.guard_ok and p.guard_ok
    assert p.off == off and ref.off == off[:-1]
    assert [w.key() for w in p.words] == [w.key() for w in ref.words]
    assert p.out == ref.out                      # the bytes, and the fill in every gap
    for i, sz in enumerate(sizes):
        assert p.out[off[i] + sz:off[i + 1]] == bytes([FILL]) * (off[i + 1] - off[i] - sz)
        if raws is not None:
            assert p.piece(i) == raws[i], i
    return p


def packed_equals_batch(target, wrap, align, lens=tuple(LENS)):
    streams, raws = exact_batch(wrap, lens)
    p = _same_as_batch(target, list(streams), wrap, [len(r) for r in raws], align, raws=raws)
    assert all(w.status == 0 for w in p.words)
    return len(streams)


def packed_shared_dict(target):
    zd = text(3000, 71)
    raws = [zd[100:100 + n] + text(n, 72 + n) for n in (0, 1, 40, 300, 5000, 40000)]
    done = 0
    for wrap in (RAW, ZLIB):
        streams = [deflate(r, wrap, 6, zdict=zd) for r in raws]
        for s, r in zip(streams, raws):
            assert inflate(s, wrap, zdict=zd) == r
        if wrap == ZLIB:
            other = deflate(raws[3], ZLIB, 6, zdict=b"another dictionary")
            streams.append(other)
        sizes = [w.size for w in target.sizes(streams, wrap, hist=len(zd))]
        assert sizes[:len(raws)] == [len(r) for r in raws]
        for align in (1, 16):
            p = _same_as_batch(target, streams, wrap, sizes, align, zdict=zd)
            assert [p.piece(i) for i in range(len(raws))] == raws
            assert all(w.status == 0 for w in p.words[:len(raws)])
            if wrap == ZLIB:
                assert p.words[-1].status == Z_DATA_ERROR and p.words[-1].size == 0     # a wrong DICTID
        done += len(streams)
    return done


# ---- 6. capacity ---------------------------------------------------------------------------------------------------------------------
def capacity(target, wrap=ZLIB, lens=(0, 1, 258, 4097, 65537), align=1):
    base = text(max(lens), 1234)
    raws = [base[:n] for n in lens for _ in range(3)] + [b""]
    streams = [deflate(r, wrap, (0, 1, 6)[i % 3]) for i, r in enumerate(raws)]
    off = aligned_scan([len(r) for r in raws], align)
    total = off[-1]
    mid = len(raws) // 2
    half = off[mid] + len(raws[mid]) // 2
    assert len(raws[mid]) > 1
    for cap in (total, total - 1, half, 0):
        p = target.packed(streams, wrap, cap, align=align)
        assert p.rc == 0 and p.guard_ok, cap
        assert p.off == off, cap                                   # ... the total among them
        fitted = 0
        for i, r in enumerate(raws):
            if off[i] + len(r) <= cap:
                assert p.words[i].key() == (len(r), 0, len(streams[i]), 0) and p.piece(i) == r, (cap, i, p.words[i])
                fitted += 1
            else:
                assert p.words[i].key() == (0, Z_BUF_ERROR, 0, 2), (cap, i, p.words[i])
                assert p.out[off[i]:min(cap, off[i + 1])] == bytes([FILL]) * (min(cap, off[i + 1]) - min(cap, off[i]))
        # (no room at all: the three empty streams at offset 0 need none; the empty stream at the very end stands at `total`)
        assert fitted == {total: len(raws), 0: 3}.get(cap, fitted) and (cap not in (total - 1, half) or 3 < fitted < len(raws))
        # the retry with the reported total completes
        q = target.packed(streams, wrap, p.off[-1], align=align)
        assert q.rc == 0 and q.guard_ok and all(w.status == 0 for w in q.words)
        assert [q.piece(i) for i in range(len(raws))] == raws
    return 4


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------
def arguments(target):
    assert target.rc_sizes(n=0) == 0 and target.rc_packed(n=0) == 0          # (the packed call also writes d_out_off[0] = 0: checked there)
    assert target.rc_sizes() == 0 and target.rc_packed() == 0
    assert target.rc_sizes(null_ctx=True) == E_ARG and target.rc_packed(null_ctx=True) == E_ARG
    for wrap in (-1, 4):
        assert target.rc_sizes(wrap=wrap) == E_ARG and target.rc_packed(wrap=wrap) == E_ARG
    for align in (0, 3, 8192):
        assert target.rc_packed(align=align) == E_ARG
    for align in (1, 2, 4096):
        assert target.rc_packed(align=align) == 0
    assert target.rc_sizes(hist=32769) == E_ARG and target.rc_sizes(hist=32768, wrap=RAW) == 0
    for wrap in (GZIP, AUTO):
        assert target.rc_packed(wrap=wrap, zdict=b"dictionary") == E_ARG
    assert target.rc_packed(wrap=ZLIB, zdict=b"dictionary") == 0 and target.rc_packed(wrap=GZIP, zdict=b"") == 0
    return 17


# ---- 8. the context's inflate-out limit belongs to the caller -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_batch():
    """twelve zlib streams of 128 KiB: under the smallest limit the setter accepts, 1 MiB, the bitmap holds the first eight"""
    raws = [text(1 << 17, 600 + i) for i in range(12)]
    return [deflate(r, ZLIB, 1) for r in raws], raws


def context_limit(target, between=None):
    """zmi_ctx_set_inflate_out_limit is the setting for calls that do not size their own scratch: calls that do (the packed call, with and
    without a dictionary; `between`: whatever else the target can run) neither use it nor change it.  The bitmap plan is a scan in stream
    order, so which streams a limit leaves out does not depend on the machine."""
    streams, raws = limit_batch()
    caps = [1 << 17] * len(raws)
    target.set_out_limit(1 << 20)

    def under_the_limit():
        b = target.batch(streams, ZLIB, caps, set_limit=False)
        assert b.rc == 0 and b.guard_ok
        assert [w.status for w in b.words] == [0] * 8 + [Z_MEM_ERROR] * 4, b.words
        assert [b.piece(i) for i in range(8)] == raws[:8]

    under_the_limit()
    if between is not None:
        between(streams, raws)
    zd = text(3000, 71)
    for zdict, ss in ((None, streams), (zd, [deflate(r, ZLIB, 1, zdict=zd) for r in raws])):
        p = target.packed(ss, ZLIB, 12 << 17, zdict=zdict)
        assert p.rc == 0 and p.guard_ok
        assert [w.status for w in p.words] == [0] * 12, p.words
        assert [p.piece(i) for i in range(12)] == raws
    under_the_limit()
    return 4


# ---- the target both test files build on: the C ABI through ctypes over a memory provider ---------------------------------------------
def bind(L):
    """the ctypes signatures these checks need"""
    import ctypes as C
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_inflate_sizes_dev.argtypes = [vp, vp, vp, vp, u32, i32, u32, u32, vp, vp, vp, vp, vp]
    L.zmi_inflate_batch_packed_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp]
    L.zmi_inflate_batch_dev_ex.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.zmi_inflate_batch_shared_dict_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.zmi_ctx_set_inflate_out_limit.argtypes = [vp, u64]
    return L


class AbiTarget:
    """mem.put(numpy array, shift) -> handle (.ptr: the device address, `shift` bytes behind a 16-byte boundary), mem.full(nbytes,
    fill) -> handle, mem.read(handle, dtype) -> numpy array, mem.stream: the stream argument.  The two calls under test go through
    _sizes / _packed, which a subclass may route through another binding."""
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem

    def _input(self, streams, shifts=None):
        import numpy as np
        shifts = shifts or [0] * len(streams)
        off, at = [], 0
        for s, sh in zip(streams, shifts):
            at = ((at + 15) & ~15) + sh
            off.append(at)
            at += len(s)
        blob = np.full(at + 64, 0x5A, dtype=np.uint8)
        for o, s in zip(off, streams):
            blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        m = self.mem
        return m.put(blob), m.put(np.array(off + [0], dtype=np.uint64)), m.put(np.array([len(s) for s in streams] + [0], dtype=np.uint32))

    def _words(self, n, size, st, used, det):
        import numpy as np
        m = self.mem
        cols = [m.read(size, np.uint32), m.read(st, np.int32), m.read(used, np.uint32), m.read(det, np.int32)]
        return [Word(*(int(c[i]) for c in cols)) for i in range(n)]

    def _sizes(self, d, off, ln, n, wrap, hist, limit, size, st, used, det):
        rc = self.L.zmi_inflate_sizes_dev(self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, hist, limit, size.ptr, st.ptr, used.ptr, det.ptr, self.mem.stream)
        assert rc == 0, rc

    def _packed(self, d, off, ln, n, wrap, zd, zlen, limit, align, out, out_cap, ooff, olen, st, used, det):
        return self.L.zmi_inflate_batch_packed_dev(self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, zd.ptr if zd is not None else None, zlen, limit, align,
                                                   out.ptr, out_cap, ooff.ptr, olen.ptr, st.ptr, used.ptr, det.ptr, self.mem.stream)

    def sizes(self, streams, wrap, hist=0, limit=0, shifts=None):
        n, m = len(streams), self.mem
        d, off, ln = self._input(streams, shifts)
        size, st, used, det = (m.full(4 * n + 4, 0x77) for _ in range(4))
        self._sizes(d, off, ln, n, wrap, hist, limit, size, st, used, det)
        return self._words(n, size, st, used, det)

    def _zdict(self, zdict):
        import numpy as np
        return None if zdict is None else self.mem.put(np.frombuffer(zdict + b"\0", dtype=np.uint8).copy(), 5)

    def _decoded(self, rc, n, off, out, out_cap, olen, st, used, det):
        import numpy as np
        host = self.mem.read(out, np.uint8).tobytes()
        return Decoded(rc, off, self._words(n, olen, st, used, det) if rc == 0 else [], host[:out_cap], host[out_cap:] == bytes([FILL]) * GUARD)

    def set_out_limit(self, nbytes):
        assert self.L.zmi_ctx_set_inflate_out_limit(self.ctx, nbytes) == 0

    def batch(self, streams, wrap, caps, zdict=None, align=1, set_limit=True):
        import numpy as np
        n, m = len(streams), self.mem
        d, off, ln = self._input(streams)
        scan = aligned_scan(caps, align)
        ooff, ocap = m.put(np.array(scan, dtype=np.uint64)), m.put(np.array(list(caps) + [0], dtype=np.uint32))
        out = m.full(scan[-1] + GUARD, FILL)
        olen, st, used, det = (m.full(4 * n + 4, 0x77) for _ in range(4))
        zd = self._zdict(zdict)
        if set_limit:
            self.set_out_limit(scan[-1] + (1 << 20))
        if zd is not None:
            rc = self.L.zmi_inflate_batch_shared_dict_dev(self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, zd.ptr, len(zdict), out.ptr, ooff.ptr, ocap.ptr,
                                                          olen.ptr, st.ptr, used.ptr, det.ptr, m.stream)
        else:
            rc = self.L.zmi_inflate_batch_dev_ex(self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, out.ptr, ooff.ptr, ocap.ptr, olen.ptr, st.ptr, used.ptr,
                                                 det.ptr, m.stream)
        return self._decoded(rc, n, scan[:-1], out, scan[-1], olen, st, used, det)

    def packed(self, streams, wrap, out_cap, align=1, zdict=None, limit=0):
        import numpy as np
        n, m = len(streams), self.mem
        d, off, ln = self._input(streams)
        out = m.full(out_cap + GUARD, FILL)
        ooff = m.full(8 * n + 16, 0x77)
        olen, st, used, det = (m.full(4 * n + 4, 0x77) for _ in range(4))
        zd = self._zdict(zdict)
        rc = self._packed(d, off, ln, n, wrap, zd, len(zdict) if zdict else 0, limit, align, out, out_cap, ooff, olen, st, used, det)
        o = m.read(ooff, np.uint64)
        assert int(o[n + 1]) == 0x7777777777777777
        return self._decoded(rc, n, [int(x) for x in o[:n + 1]], out, out_cap, olen, st, used, det)

    def rc_sizes(self, wrap=ZLIB, hist=0, null_ctx=False, n=1):
        s = deflate(b"abc", RAW if wrap == RAW else (GZIP if wrap == GZIP else ZLIB))
        d, off, ln = self._input([s])
        size, st = self.mem.full(8, 0x77), self.mem.full(8, 0x77)
        return self.L.zmi_inflate_sizes_dev(None if null_ctx else self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, hist, 0, size.ptr, st.ptr, None, None,
                                            self.mem.stream)

    def rc_packed(self, wrap=ZLIB, align=1, zdict=None, null_ctx=False, n=1):
        import numpy as np
        s = deflate(b"abc", RAW if wrap == RAW else (GZIP if wrap == GZIP else ZLIB))
        d, off, ln = self._input([s])
        m = self.mem
        out, ooff, olen, st = m.full(64, FILL), m.full(24, 0x77), m.full(8, 0x77), m.full(8, 0x77)
        zd = self._zdict(zdict)
        rc = self.L.zmi_inflate_batch_packed_dev(None if null_ctx else self.ctx, d.ptr, off.ptr, ln.ptr, n, wrap, zd.ptr if zd is not None else None,
                                                 len(zdict) if zdict else 0, 0, align, out.ptr, 64, ooff.ptr, olen.ptr, st.ptr, None, None, m.stream)
        if rc == 0:
            o = m.read(ooff, np.uint64)
            assert [int(x) for x in o[:n + 1]] == ([0, (3 + align - 1) & ~(align - 1)] if n else [0]) and int(o[n + 1]) == 0x7777777777777777
            if n:
                assert (int(m.read(st, np.int32)[0]), m.read(out, np.uint8).tobytes()[:3]) == (0, b"abc")
        return rc
