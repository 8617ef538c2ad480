"""Checks of random access into one deflate stream (zmi_inflate_stream_index_dev / zmi_inflate_ranges_dev, include/zmi355.h), shared by
tests/test_emu_ranges.py (CPU, the emulator build through ctypes) and tests/test_gpu_ranges.py (the MI355X).

The judge of bytes is Python's zlib on the CPU; the judge of the index is the greedy rule applied on the host to the output offsets
of the pieces, which a small block walker (F1), the piece size (F2) or the flush points (F3) give.

A Target wraps the C ABI over a memory provider (mem.put / mem.full / mem.read / mem.stream, as in inflate_sizes_checks.py).
"""
import functools
import hashlib
import os
import random
import zlib

import numpy as np

RAW, ZLIB, GZIP, AUTO = 0, 1, 2, 3
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
HEADER = {RAW: 0, ZLIB: 2, GZIP: 10}
Z_DATA_ERROR, Z_BUF_ERROR, E_ARG = -3, -5, -103
WIN = 32768
FILL = 0xA5
GUARD = 64
POM = 1 << 17
SPANS = (1, 10000, 40000, 1 << 40)
DEFAULT_SCRATCH = 8 << 30


def bind(L):
    """the ctypes signatures these checks need"""
    import ctypes as C
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    L.zmi_deflate_stream_bound.restype = u64
    L.zmi_deflate_stream_bound.argtypes = [u64, u32, i32]
    L.zmi_deflate_stream_dev.argtypes = [vp, vp, u64, u32, i32, i32, i32, u32, vp, u64, vp, vp, vp, vp]
    L.zmi_inflate_stream_bits_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_stream_find_cuts_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    L.zmi_stream_find_blocks_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    L.zmi_inflate_stream_index_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, u32, vp, vp, vp]
    L.zmi_inflate_ranges_dev.argtypes = [vp, vp, u64, vp, vp, vp, u32, u64, vp, vp, u32, u32, vp, vp, u64, vp, vp, vp]
    return L


# ---- data and streams ----------------------------------------------------------------------------------------------------------------
def text(n, seed):
    """the word text of tests/test_emu_stream_inflate_blocks.py (_text), restated"""
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
        if rnd.random() < 0.01:
            out += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 40)))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def data():
    return text(150000, 9)


def host_deflate(raw, wrap, level=6, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap], mem)
    return c.compress(raw) + c.flush()


# the block walker: (bit offset of the block's first header bit, BTYPE, output offset) of every block of a raw deflate stream
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def _huff(lengths):
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0], code, nxt = 0, 0, [0] * 16
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    t = {}
    for s, l in enumerate(lengths):
        if l:
            t[(l, int(format(nxt[l], "0%db" % l)[::-1], 2))] = s
            nxt[l] += 1
    return t, min([l for l in lengths if l] or [1])


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos = raw, 0

    def get(self, n, keep=False):
        p = self.pos
        v = (int.from_bytes(self.raw[p >> 3:(p >> 3) + 4], "little") >> (p & 7)) & ((1 << n) - 1)
        if not keep:
            self.pos += n
        return v

    def sym(self, table):
        t, lo = table
        w = self.get(15, keep=True)
        for l in range(lo, 16):
            s = t.get((l, w & ((1 << l) - 1)))
            if s is not None:
                self.pos += l
                return s
        raise ValueError("bad code at bit %d" % self.pos)


def walk(raw):
    fixed = (_huff([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _huff([5] * 30))
    b, out, produced = _Bits(raw), [], 0
    while True:
        at, last, typ = b.pos, b.get(1), b.get(2)
        out.append((at, typ, produced))
        if typ == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.get(16)
            b.pos += 16 + 8 * n
            produced += n
        else:
            ll, dd = fixed
            if typ == 2:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_ORDER[i]] = b.get(3)
                ct, ls = _huff(cl), []
                while len(ls) < hlit + hdist:
                    s = b.sym(ct)
                    ls += [s] if s < 16 else ([ls[-1]] * (3 + b.get(2)) if s == 16 else [0] * ((3 + b.get(3)) if s == 17 else (11 + b.get(7))))
                ll, dd = _huff(ls[:hlit]), _huff(ls[hlit:])
            while True:
                s = b.sym(ll)
                if s == 256:
                    break
                if s < 256:
                    produced += 1
                else:
                    produced += _LBASE[s - 257] + b.get(_LEXTRA[s - 257])
                    d = b.sym(dd)
                    b.pos += max(0, d // 2 - 1)
        if last:
            return out, produced


class Fixture:
    """stream, wrap, cuts (bits), pom, payload; offs: the output offset at every cut (None where only the device knows)"""
    def __init__(self, name, stream, wrap, cuts, payload, offs=None, pom=POM):
        self.name, self.stream, self.wrap, self.cuts, self.payload, self.offs, self.pom = name, stream, wrap, cuts, payload, offs, pom


_FIX = {}


def fixture(target, name):
    """F1-raw / F1-zlib / F1-gzip / F2 / F3 / F4 / F5, made once (the cuts come from the library's own proposal calls)"""
    if name in _FIX:
        return _FIX[name]
    if name.startswith("F1"):
        wrap = {"raw": RAW, "zlib": ZLIB, "gzip": GZIP}[name[3:]]
        s = host_deflate(data(), wrap, 6, 2)
        cuts = target.find_blocks(s, wrap, 1)
        blocks, produced = walk(host_deflate(data(), RAW, 6, 2))
        assert produced == len(data()) and len(cuts) > 80
        at = {8 * HEADER[wrap] + b: o for b, _, o in blocks}
        f = Fixture(name, s, wrap, cuts, data(), [at[c] for c in cuts])
        assert sum(1 for c in cuts if c & 7) > 40 and f.offs[0] == 0
    elif name == "F2":
        s, idx = target.deflate_stream(data(), 16384, GZIP)
        f = Fixture(name, s, GZIP, [8 * x for x in idx], data(), [16384 * i for i in range(len(idx))], pom=16384)
        assert zlib.decompress(s, 31) == data() and len(idx) == 10
    elif name == "F3":
        block = random.Random(33).getrandbits(8 * 20000).to_bytes(20000, "little")
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        parts = []
        for k in range(4):
            parts.append(c.compress(block) + (c.flush(zlib.Z_SYNC_FLUSH) if k < 3 else c.flush()))
        s = b"".join(parts)
        assert len(parts[0]) > 20000 and all(len(p) < 400 for p in parts[1:])
        cuts = [0] + [8 * sum(len(p) for p in parts[:k]) for k in (1, 2, 3)]
        f = Fixture(name, s, RAW, cuts, block * 4, [0, 20000, 40000, 60000])
        try:   # piece 2 without its window: "invalid distance too far back"
            zlib.decompressobj(-15).decompress(s[cuts[2] // 8:])
            raise AssertionError("piece 2 of F3 decodes without history")
        except zlib.error as e:
            assert "distance" in str(e)
    elif name == "F4":
        s = host_deflate(data(), GZIP, 0)
        f = Fixture(name, s, GZIP, [8 * HEADER[GZIP]], data(), [0], pom=1 << 18)
    elif name == "F5":
        s = zlib.compress(b"")
        f = Fixture(name, s, ZLIB, [16], b"", [0], pom=4096)
    else:
        raise KeyError(name)
    _FIX[name] = f
    return f


class Index:
    def __init__(self, rc, n, bit, out, win, max_gap, words, data, canary):
        self.rc, self.n, self.bit, self.out, self.win, self.max_gap = rc, n, bit, out, win, max_gap
        self.words, self.data, self.canary = words, data, canary   # words: (status, detail, out_len, in_used)

    def key(self):
        return (self.n, tuple(self.bit), tuple(self.out), self.max_gap, self.words)


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem

    def ok(self, rc, what):
        assert rc == 0, "%s: %d %s" % (what, rc, self.L.zmi_last_error().decode())

    def _bytes(self, b, shift=0):
        return self.mem.put(np.frombuffer(bytes(b) + b"\0" * 16, dtype=np.uint8), shift)

    def scratch_limit(self, nbytes):
        self.ok(self.L.zmi_ctx_set_scratch_limit(self.ctx, nbytes), "scratch limit")

    def _find(self, fn, s, wrap, min_gap, cap):
        m = self.mem
        inp, cuts, cnt = self._bytes(s), m.full(8 * cap, 0), m.full(4, 0xFF)
        self.ok(fn(self.ctx, inp.ptr, len(s), wrap, min_gap, cuts.ptr, cap, cnt.ptr, m.stream), "find")
        n = int(m.read(cnt, np.uint32)[0])
        assert n <= cap
        return [int(x) for x in m.read(cuts, np.uint64)[:n]]

    def find_blocks(self, s, wrap, min_gap=1, cap=4096):
        return self._find(self.L.zmi_stream_find_blocks_dev, s, wrap, min_gap, cap)

    def find_cuts(self, s, wrap, min_gap=1, cap=4096):
        return self._find(self.L.zmi_stream_find_cuts_dev, s, wrap, min_gap, cap)

    def deflate_stream(self, raw, piece, wrap, flags=0, level=6):
        L, m, n = self.L, self.mem, len(raw)
        cap = int(L.zmi_deflate_stream_bound(n, piece, wrap))
        pieces = max(1, -(-n // piece))
        inp, out, olen, st, idx = self._bytes(raw), m.full(cap + 64, 0), m.full(8, 0), m.full(4, 77), m.full(8 * (pieces + 1), 0)
        self.ok(L.zmi_deflate_stream_dev(self.ctx, inp.ptr, n, piece, level, 0, wrap, flags, out.ptr, cap, olen.ptr, idx.ptr, st.ptr, m.stream),
                "zmi_deflate_stream_dev")
        assert int(m.read(st, np.int32)[0]) == 0
        return m.read(out, np.uint8)[:int(m.read(olen, np.uint64)[0])].tobytes(), [int(x) for x in m.read(idx, np.uint64)[:pieces]]

    def _words(self, w):
        a = self.mem.read(w, np.uint64)
        st, det = (int(x) for x in a[2:3].view(np.int32))
        return (st, det, int(a[0]), int(a[1]))

    def inflate_bits(self, s, wrap, cuts, pom, out_cap):
        """-> ((status, detail, out_len, in_used), bytes, canary intact)"""
        m = self.mem
        inp, cu, out, w = self._bytes(s), m.put(np.array(cuts, dtype=np.uint64)), m.full(out_cap + 256, 0x5A), m.full(32, 0)
        self.ok(self.L.zmi_inflate_stream_bits_dev(self.ctx, inp.ptr, len(s), wrap, cu.ptr, len(cuts), pom, out.ptr, out_cap, w.ptr, w.ptr + 8,
                                                   w.ptr + 16, w.ptr + 20, m.stream), "inflate bits")
        words, host = self._words(w), m.read(out, np.uint8)
        return words, host[:min(words[2], out_cap)].tobytes(), bool((host[out_cap:] == 0x5A).all())

    def index_raw(self, s, wrap, cuts, pom, out_cap, span, ix_cap, win=True, null=None, null_ctx=False):
        m = self.mem
        inp, cu, out, w = self._bytes(s), m.put(np.array(cuts, dtype=np.uint64)), m.full(out_cap + 256, 0x5A), m.full(32, 0)
        ib, io = m.full(8 * max(ix_cap, 1) + 64, 0x77), m.full(8 * (max(ix_cap, 1) + 1) + 64, 0x77)
        iw = m.full(max(ix_cap, 1) * WIN + 64, 0x77) if win else None
        npts, mg = m.full(4, 0x77), m.full(8, 0x77)
        ptr = {"bit": ib.ptr, "out": io.ptr, "n": npts.ptr, "gap": mg.ptr}
        if null:
            ptr[null] = None
        rc = self.L.zmi_inflate_stream_index_dev(None if null_ctx else self.ctx, inp.ptr, len(s), wrap, cu.ptr, len(cuts), pom, out.ptr, out_cap,
                                                 w.ptr, w.ptr + 8, w.ptr + 16, w.ptr + 20, span, ptr["bit"], ptr["out"], iw.ptr if win else None, ix_cap,
                                                 ptr["n"], ptr["gap"], m.stream)
        if rc != 0:
            return Index(rc, 0, [], [], None, 0, None, b"", True)
        n = int(m.read(npts, np.uint32)[0])
        assert n <= ix_cap
        words, host = self._words(w), m.read(out, np.uint8)
        bits, outs = m.read(ib, np.uint64), m.read(io, np.uint64)
        # nothing behind the entries the call owns is written
        assert (bits[ix_cap:] == 0x7777777777777777).all() and (outs[ix_cap + 1:] == 0x7777777777777777).all()
        wins = None
        if win:
            wh = m.read(iw, np.uint8)
            assert (wh[ix_cap * WIN:] == 0x77).all()
            wins = wh[:n * WIN].reshape(n, WIN)
        return Index(0, n, [int(x) for x in bits[:n]], [int(x) for x in outs[:n + 1]] if n else [], wins, int(m.read(mg, np.uint64)[0]), words,
                     host[:min(words[2], out_cap)].tobytes(), bool((host[out_cap:] == 0x5A).all()))

    def index(self, f, span, ix_cap=None, win=True, out_cap=None):
        return self.index_raw(f.stream, f.wrap, f.cuts, f.pom, len(f.payload) + 7 if out_cap is None else out_cap, span, ix_cap or len(f.cuts), win)

    def ranges(self, s, ix, los, lens, max_len=None, max_gap=None, use_off=True, odd=False, in_len=None, win=True, n_points=None, bit=None, out=None,
               null=None, null_ctx=False):
        """-> (rc, got, status, the bytes of every range, intact): region i = len_i bytes behind a GUARD, everything pre-filled; intact =
        no byte outside [off_i, off_i + got_i) changed"""
        m, n = self.mem, len(los)
        max_len = max(lens + [1]) if max_len is None else max_len
        if use_off:
            offs, at = [], GUARD
            for l in lens:
                offs.append(at)
                at += l + GUARD
            total, stride = at, 0
        else:
            stride = max(lens + [1]) + GUARD
            offs, total = [i * stride for i in range(n)], n * stride + GUARD
        inp = self._bytes(s)
        ib = m.put(np.array((bit if bit is not None else ix.bit) + [0], dtype=np.uint64))
        io = m.put(np.array(out if out is not None else ix.out, dtype=np.uint64))
        iw = m.put(np.ascontiguousarray(ix.win).reshape(-1)) if (win and ix.win is not None) else None
        lo_d, ln_d = m.put(np.array(list(los) + [0], dtype=np.uint64)), m.put(np.array(list(lens) + [0], dtype=np.uint32))
        od = m.put(np.array(offs + [0], dtype=np.uint64))
        buf = m.put(np.full(total + 16, FILL, dtype=np.uint8), 1 if odd else 0)
        got, st = m.full(4 * n + 4, 0x77), m.full(4 * n + 4, 0x77)
        ptr = {"bit": ib.ptr, "out": io.ptr, "lo": lo_d.ptr, "len": ln_d.ptr, "dst": buf.ptr, "got": got.ptr, "st": st.ptr}
        if null:
            ptr[null] = None
        rc = self.L.zmi_inflate_ranges_dev(None if null_ctx else self.ctx, inp.ptr, len(s) if in_len is None else in_len, ptr["bit"], ptr["out"],
                                           iw.ptr if iw is not None else None, ix.n if n_points is None else n_points,
                                           ix.max_gap if max_gap is None else max_gap, ptr["lo"], ptr["len"], n, max_len, ptr["dst"],
                                           od.ptr if use_off else None, stride, ptr["got"], ptr["st"], m.stream)
        if rc != 0:
            return rc, [], [], [], True
        g, t = m.read(got, np.uint32), m.read(st, np.int32)
        assert int(g[n]) == 0x77777777 and int(t[n]) == 0x77777777
        host = m.read(buf, np.uint8)
        g, t = [int(x) for x in g[:n]], [int(x) for x in t[:n]]
        want = np.full(total + 16, FILL, dtype=np.uint8)
        for o, k in zip(offs, g):
            want[o:o + k] = host[o:o + k]
        return 0, g, t, [host[o:o + k].tobytes() for o, k in zip(offs, g)], bool((host == want).all())


# ---- 1. the index is exact ---------------------------------------------------------------------------------------------------------
def greedy(points, span):
    """points: [(bit, out)] in stream order -> the greedy thinning by output offset"""
    keep = [points[0]]
    for p in points[1:]:
        if p[1] >= keep[-1][1] + max(span, 1):
            keep.append(p)
    return keep


def _check_index(ix, f, want, total, cap=None):
    want = want[:cap] if cap else want
    assert ix.rc == 0 and ix.words == (0, 0, total, len(f.stream)) and ix.data == f.payload and ix.canary, (f.name, ix.words)
    assert list(zip(ix.bit, ix.out[:-1])) == want, (f.name, len(want), ix.n)
    assert ix.out[-1] == total and all(a < b for a, b in zip(ix.out, ix.out[1:-1])) and ix.out[0] == 0 and ix.bit[0] == f.cuts[0]
    assert ix.max_gap == max(b - a for a, b in zip(ix.out, ix.out[1:]))
    if ix.win is not None:
        for k, o in enumerate(ix.out[:-1]):
            w = f.payload[max(0, o - WIN):o]
            assert ix.win[k].tobytes() == bytes(WIN - len(w)) + w, (f.name, k, o)


def index_exact(target, name, setenv=None, spans=SPANS, variants=True):
    """-> the number of index builds checked"""
    f = fixture(target, name)
    total = len(f.payload)
    ref = target.inflate_bits(f.stream, f.wrap, f.cuts, f.pom, total + 7)
    assert ref[0] == (0, 0, total, len(f.stream)) and ref[1] == f.payload and ref[2]
    every = greedy(list(zip(f.cuts, f.offs)), 1)          # every piece start that advances the output
    one = target.index(f, 1)
    _check_index(one, f, every, total)
    assert (one.words, one.data) == (ref[0], ref[1])
    done = 1
    span1 = list(zip(one.bit, one.out[:-1]))
    for span in spans[1:]:
        ix = target.index(f, span)
        _check_index(ix, f, greedy(span1, span), total)
        done += 1
    if len(every) > 16:
        assert 1 < len(greedy(span1, 10000)) < len(greedy(span1, 1)) and len(greedy(span1, 40000)) >= 3 and len(greedy(span1, 1 << 40)) == 1
        assert any(0 < o < WIN for _, o in greedy(span1, 10000))   # a partial window
    if not variants:
        return done
    half = max(1, len(every) // 2)
    ix = target.index(f, 1, ix_cap=half)
    _check_index(ix, f, every, total, cap=half)
    assert ix.n == half and (len(every) == 1 or ix.max_gap == total - every[half - 1][1] > one.max_gap)
    again = target.index(f, 1)
    assert again.key() == one.key() and (again.win == one.win).all()
    nowin = target.index(f, 1, win=False)
    assert nowin.key() == one.key() and nowin.win is None
    done += 3
    if setenv is not None:
        setenv("ZMI_STREAM_GROUP", "7")
        g7 = target.index(f, 10000)
        setenv("ZMI_STREAM_GROUP", None)
        target.scratch_limit(64 << 20)
        try:
            f1m = Fixture(f.name, f.stream, f.wrap, f.cuts, f.payload, f.offs, pom=1 << 20)   # 64 MiB hold 19 regions of 1 MiB
            lim = target.index(f1m, 10000)
        finally:
            target.scratch_limit(DEFAULT_SCRATCH)
        base = target.index(f, 10000)
        for other in (g7, lim):
            assert other.key() == base.key() and (other.win == base.win).all() and other.data == base.data
        done += 3
    return done


# ---- 2. a void index -----------------------------------------------------------------------------------------------------------------
def void_index(target):
    f = fixture(target, "F1-gzip")
    total = len(f.payload)
    bad = bytearray(f.stream)
    bad[-6] ^= 0x10                                         # the CRC-32 of the trailer
    moved = list(f.cuts)
    moved[len(moved) // 2] += 1
    cases = [target.index_raw(bytes(bad), f.wrap, f.cuts, f.pom, total + 7, 10000, len(f.cuts)),
             target.index_raw(f.stream, f.wrap, moved, f.pom, total + 7, 10000, len(f.cuts)),
             target.index_raw(f.stream, f.wrap, f.cuts, f.pom, total - 1, 10000, len(f.cuts))]
    for ix in cases:
        assert ix.rc == 0 and ix.n == 0 and ix.words[0] != 0 and ix.canary, ix.words
    assert cases[0].words[:2] == (Z_DATA_ERROR, 7) and cases[1].words[1] & 0xFF == 3 and cases[2].words[:3] == (Z_BUF_ERROR, 9, total)
    return len(cases)


# ---- 3. ranges are exact -----------------------------------------------------------------------------------------------------------------
_IX = {}


def built(target, name, span):
    """the index of a fixture at a span, built once"""
    if (name, span) not in _IX:
        ix = target.index(fixture(target, name), span)
        assert ix.rc == 0 and ix.words[0] == 0 and ix.n >= 1
        _IX[(name, span)] = ix
    return _IX[(name, span)]


def seeded_ranges(total, n=50, top=40000, seed=5):
    r = random.Random(seed)
    return [(r.randrange(0, total), r.randint(1, top)) for _ in range(n)]


def fixed_ranges(ix, total):
    p = ix.out[ix.n // 2] if ix.n > 2 else total // 2
    return [(0, 1), (0, total), (total - 1, 1), (total, 5), (total - 3, 10), (p, 1), (p - 1, 2), (p + 32767, 3), (total // 3, 0)]


def _check_ranges(res, ranges, payload, what):
    rc, got, st, chunks, intact = res
    assert rc == 0 and intact, what
    for i, (lo, ln) in enumerate(ranges):
        want = payload[lo:lo + ln]
        assert (got[i], st[i]) == (len(want), 0) and chunks[i] == want, (what, i, lo, ln, got[i], st[i])
    return len(ranges)


def ranges_exact(target, name, span, layouts=((True, False), (False, False), (True, True)), n=50):
    """layouts: (offset table or stride, d_out at an odd address)"""
    f = fixture(target, name)
    ix, total = built(target, name, span), len(f.payload)
    ranges = fixed_ranges(ix, total) + seeded_ranges(total, n)
    done = 0
    for use_off, odd in layouts:
        res = target.ranges(f.stream, ix, [a for a, _ in ranges], [b for _, b in ranges], use_off=use_off, odd=odd)
        done += _check_ranges(res, ranges, f.payload, (name, span, use_off, odd))
    return done


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
def _digest(res, order=None):
    rc, got, st, chunks, intact = res
    assert rc == 0 and intact
    order = order if order is not None else list(range(len(got)))
    rows = sorted(zip(order, got, st, chunks))
    h = hashlib.sha256()
    for _, g, s, c in rows:
        h.update(b"%d %d " % (g, s) + c)
    return h.hexdigest()


_DIGEST = {}


def independence(target, name="F1-gzip", span=40000, n=50, one_by_one=True, two_regions=True):
    f = fixture(target, name)
    ix, total = built(target, name, span), len(f.payload)
    ranges = seeded_ranges(total, n) + [(total - 3, 10), (total, 5), (7, 0)]
    los, lens = [a for a, _ in ranges], [b for _, b in ranges]
    base = _digest(target.ranges(f.stream, ix, los, lens))
    assert _DIGEST.setdefault((name, span, n), base) == base            # ... under every decode selection the tests run with
    m = len(ranges)
    assert _digest(target.ranges(f.stream, ix, los[::-1], lens[::-1]), list(range(m))[::-1]) == base
    done = 2
    if one_by_one:
        rows = [target.ranges(f.stream, ix, [a], [b], max_len=max(lens)) for a, b in ranges]
        assert all(r[0] == 0 and r[4] for r in rows)
        assert _digest((0, [r[1][0] for r in rows], [r[2][0] for r in rows], [r[3][0] for r in rows], True)) == base
        done += 1
    if two_regions:
        target.scratch_limit(64 << 20)
        try:   # 24 MiB of claimed gap: 27 MiB of scratch a range, two regions per launch group
            assert _digest(target.ranges(f.stream, ix, los, lens, max_gap=24 << 20)) == base
        finally:
            target.scratch_limit(DEFAULT_SCRATCH)
        done += 1
    return done


# ---- 5. windows matter and may be withheld ----------------------------------------------------------------------------------------------------
def windows(target):
    f = fixture(target, "F3")
    ix = target.index(f, 1)
    assert ix.rc == 0 and ix.words[0] == 0 and list(zip(ix.bit, ix.out[:-1])) == list(zip(f.cuts, f.offs)) and ix.out[-1] == 80000
    ranges = [(0, 500), (19990, 20), (20000, 100), (40010, 1000), (45000, 15000), (60000, 20000), (100, 79900)]
    los, lens = [a for a, _ in ranges], [b for _, b in ranges]
    _check_ranges(target.ranges(f.stream, ix, los, lens), ranges, f.payload, "F3 with windows")
    rc, got, st, chunks, intact = target.ranges(f.stream, ix, los, lens, win=False)
    assert rc == 0 and intact
    for i, (lo, ln) in enumerate(ranges):
        if lo < 20000:                                      # entered at point 0: everything it refers to is its own output
            assert (got[i], st[i], chunks[i]) == (ln, 0, f.payload[lo:lo + ln]), i
        else:                                               # pieces 1 .. 3 are copies of what lies in front of them
            assert (got[i], st[i]) == (0, Z_DATA_ERROR), (i, got[i], st[i])
    assert (got[3], st[3]) == (0, Z_DATA_ERROR)             # a range inside piece 2
    return len(ranges)


# ---- 6. truncation --------------------------------------------------------------------------------------------------------------------------
def truncation(target, name="F1-gzip", span=10000):
    f = fixture(target, name)
    ix, total = built(target, name, span), len(f.payload)
    k = ix.n - 2
    assert k >= 3
    ranges = [(ix.out[1] + 5, 3000), (ix.out[2] - 10, 20), (100, 700), (ix.out[k] + 10, ix.out[k + 1] - ix.out[k] - 20)]
    los, lens = [a for a, _ in ranges], [b for _, b in ranges]
    full = target.ranges(f.stream, ix, los, lens)
    _check_ranges(full, ranges, f.payload, "untruncated")
    cut = ((ix.bit[k] >> 3) + (ix.bit[k + 1] >> 3)) // 2     # inside the extent of the last range only
    assert (ix.bit[k] >> 3) + 8 < cut < (ix.bit[k + 1] >> 3) - 8 and (ix.bit[3] >> 3) + 1 < cut
    rc, got, st, chunks, intact = target.ranges(f.stream[:cut] + bytes(64), ix, los, lens, in_len=cut)
    assert rc == 0 and intact
    assert (got[-1], st[-1]) == (0, Z_BUF_ERROR), (got[-1], st[-1])
    assert (got[:-1], st[:-1], chunks[:-1]) == (full[1][:-1], full[2][:-1], full[3][:-1])
    return len(ranges)


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------------
def arguments(target):
    f = fixture(target, "F1-gzip")
    ix, total = built(target, "F1-gzip", 10000), len(f.payload)
    assert ix.n >= 6
    done = 0
    # as the return value
    R = lambda **kw: target.ranges(f.stream, ix, [10], [20], **kw)[0]
    assert R() == 0
    for kw in ({"null_ctx": True}, {"null": "bit"}, {"null": "out"}, {"null": "lo"}, {"null": "len"}, {"null": "dst"}, {"null": "got"}, {"null": "st"},
               {"n_points": 0}, {"max_len": 0}, {"max_len": (1 << 30) + 1}, {"max_gap": (1 << 30) + 1}):
        assert R(**kw) == E_ARG, kw
        done += 1
    assert R(max_len=1 << 30, max_gap=ix.max_gap) == 0
    assert target.ranges(f.stream, ix, [], [])[0] == 0 and target.ranges(f.stream, ix, [], [], null="lo")[0] == 0     # n_ranges == 0: a no-op
    I = lambda **kw: target.index_raw(f.stream, f.wrap, f.cuts, f.pom, total + 7, 10000, kw.pop("ix_cap", 8), **kw).rc
    assert I() == 0
    for kw in ({"ix_cap": 0}, {"null": "bit"}, {"null": "out"}, {"null": "n"}, {"null": "gap"}, {"null_ctx": True}):
        assert I(**kw) == E_ARG, kw
        done += 1
    # in the status words
    p = ix.out[3]
    ranges = [(p + 5, 100), (5, 50)]
    los, lens = [a for a, _ in ranges], [b for _, b in ranges]
    ok = target.ranges(f.stream, ix, los, lens)
    _check_ranges(ok, ranges, f.payload, "arguments")

    def words(**kw):
        rc, got, st, chunks, intact = target.ranges(f.stream, ix, kw.pop("los", los), kw.pop("lens", lens), **kw)
        assert rc == 0 and intact
        return list(zip(got, st))

    assert words(lens=[100, 51], max_len=50) == [(0, E_ARG), (0, E_ARG)] and words(lens=[100, 50], max_len=50) == [(0, E_ARG), (50, 0)]
    true_gap = max(b - a for a, b in zip(ix.out, ix.out[1:]))
    assert ix.max_gap == true_gap
    small = ix.out[4] - ix.out[3] - 1                         # too small for the gap behind point 3
    assert words(max_gap=small)[0] == (0, E_ARG)
    assert words(los=[ix.out[4] - 1, 5], lens=[1, 50], max_gap=ix.out[4] - ix.out[3])[0] == (1, 0)
    down = list(ix.out)
    down[4] = down[3]                                         # the entries around the point do not ascend
    assert words(out=down, max_gap=1 << 30) == [(0, E_ARG), (50, 0)]
    bits = list(ix.bit)
    bits[4] = bits[3]                                         # the point that ends the extent lies at the one it starts from
    assert words(bit=bits) == [(0, E_ARG), (50, 0)]
    at = 8 * len(f.stream)
    bits = list(ix.bit)
    bits[3] = at                                              # a bit position at 8 * in_len
    assert words(bit=bits) == [(0, E_ARG), (50, 0)]
    done += 7
    return done
