"""CPU tests of the single-stream inflate for streams WITHOUT flush points: zmi_stream_find_blocks_dev (the block scan of
csrc/blockscan.hip as ordered proposals at bit positions) and zmi_inflate_stream_bits_dev (the stream pipeline with cuts at bit
positions; include/zmi355.h, csrc/inflate.hip, zmi_api.hip) on the emulator build.
The streams are Python zlib's: a small memLevel shrinks its symbol buffer, so 150 kB of text give dozens of dynamic blocks, most
of them at a non-zero bit offset.  A small block walker (below) says where the blocks really start.  What is checked: the proposals
are exactly the dynamic block starts and their greedy thinning, round trips through them, byte cuts given as bit cuts against
zmi_inflate_stream_dev, mixed proposals, cuts off by one bit, false proposals inside a stored block, every error the API names,
and independence of launch groups, scratch limit and scan window."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libzmi355_emu.so")
WBITS = {0: -15, 1: 15, 2: 31}
HEADER = {0: 0, 1: 2, 2: 10}
TRAILER = {0: 0, 1: 4, 2: 8}
INDEPENDENT = 1
Z_DATA_ERROR, Z_BUF_ERROR = -3, -5
SI_TRUNC, SI_CUT, SI_PIECE, SI_CHECK, SI_OUT = 2, 3, 4, 7, 9
CONFIGS = [(6, 4), (6, 2), (6, 1), (1, 4)]   # (level, memLevel)
POM = 1 << 17


def _p(a):
    return a.ctypes.data


def _bind(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_ctx_create.argtypes = [C.POINTER(vp), i32]
    L.zmi_ctx_destroy.argtypes = [vp]
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    L.zmi_deflate_stream_bound.restype = u64
    L.zmi_deflate_stream_bound.argtypes = [u64, u32, i32]
    L.zmi_deflate_stream_dev.argtypes = [vp, vp, u64, u32, i32, i32, i32, u32, vp, u64, vp, vp, vp, vp]
    L.zmi_inflate_stream_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_inflate_stream_bits_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_stream_find_cuts_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    L.zmi_stream_find_blocks_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    return L


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu"), "libzmi355_emu.so"], check=True)
    return _bind(C.CDLL(EMU))


class _Ctx:
    def __init__(self, L):
        self.L = L
        self.ctx = C.c_void_p()
        assert L.zmi_ctx_create(C.byref(self.ctx), 0) == 0

    def close(self):
        self.L.zmi_ctx_destroy(self.ctx)

    def ok(self, rc, what):
        assert rc == 0, "%s: %d %s" % (what, rc, self.L.zmi_last_error().decode())

    def deflate(self, data, piece, wrap, flags=0, level=6):
        L, n = self.L, len(data)
        inp = np.frombuffer(bytes(data) + b"\0" * 16, dtype=np.uint8).copy()
        cap = int(L.zmi_deflate_stream_bound(n, piece, wrap))
        out = np.zeros(cap + 64, dtype=np.uint8)
        olen = np.zeros(1, dtype=np.uint64)
        st = np.full(1, 77, dtype=np.int32)
        idx = np.zeros(max(1, -(-n // piece)) + 1, dtype=np.uint64)
        self.ok(L.zmi_deflate_stream_dev(self.ctx, _p(inp), n, piece, level, 0, wrap, flags, _p(out), cap, _p(olen), _p(idx), _p(st), None),
                "zmi_deflate_stream_dev")
        assert int(st[0]) == 0
        return bytes(out[:int(olen[0])]), [int(x) for x in idx[:-1]]

    def _find(self, fn, s, wrap, min_gap, cap):
        inp = np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy()
        cuts = np.zeros(max(cap, 1), dtype=np.uint64)
        cnt = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
        self.ok(fn(self.ctx, _p(inp), len(s), wrap, min_gap, _p(cuts), cap, _p(cnt), None), "find")
        assert int(cnt[0]) <= cap
        return [int(x) for x in cuts[:int(cnt[0])]]

    def find_cuts(self, s, wrap, min_gap=1, cap=4096):
        return self._find(self.L.zmi_stream_find_cuts_dev, s, wrap, min_gap, cap)

    def find_blocks(self, s, wrap, min_gap=1, cap=4096):
        return self._find(self.L.zmi_stream_find_blocks_dev, s, wrap, min_gap, cap)

    def _inflate(self, fn, s, wrap, cuts, piece_out_max, out_cap):
        """-> (status, detail, out_len, in_used, output bytes, canary intact)"""
        inp = np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy()
        cu = np.array(cuts, dtype=np.uint64)
        out = np.full(out_cap + 256, 0x5A, dtype=np.uint8)
        w = np.zeros(4, dtype=np.uint64)   # out_len | in_used | status, detail (int32)
        self.ok(fn(self.ctx, _p(inp), len(s), wrap, _p(cu), len(cuts), piece_out_max, _p(out), out_cap, _p(w), _p(w) + 8, _p(w) + 16,
                   _p(w) + 20, None), "inflate")
        st, det = (int(x) for x in w[2:3].view(np.int32))
        olen = int(w[0])
        return st, det, olen, int(w[1]), bytes(out[:min(olen, out_cap)]), bool((out[out_cap:] == 0x5A).all())

    def inflate(self, s, wrap, cuts, piece_out_max, out_cap):
        return self._inflate(self.L.zmi_inflate_stream_dev, s, wrap, cuts, piece_out_max, out_cap)

    def inflate_bits(self, s, wrap, cuts, piece_out_max, out_cap):
        return self._inflate(self.L.zmi_inflate_stream_bits_dev, s, wrap, cuts, piece_out_max, out_cap)


@pytest.fixture(scope="module")
def ctx(lib):
    e = _Ctx(lib)
    yield e
    e.close()


def _text(n, seed):
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
        if rnd.random() < 0.01:
            out += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 40)))
    return bytes(out[:n])


def _zlib_stream(data, wrap, points, mode=zlib.Z_SYNC_FLUSH, level=6, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap], mem)
    out, at = [], 0
    for p in sorted(points) + [len(data)]:
        out.append(c.compress(data[at:p]))
        if p < len(data):
            out.append(c.flush(mode))
        at = p
    out.append(c.flush())
    return b"".join(out)


# ---- the block walker: code lengths and symbols are decoded only to find where each block starts and what type it is -------------
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _huff(lengths):
    """{(length, the code as its bits arrive, first bit lowest): symbol}, shortest length"""
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


_FIXED = None


def _walk(raw):
    """[(bit offset of the block's first header bit, BTYPE)] of a raw deflate stream"""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_huff([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _huff([5] * 30))
    b, out = _Bits(raw), []
    while True:
        at, last, typ = b.pos, b.get(1), b.get(2)
        out.append((at, typ))
        if typ == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.get(16)
            b.pos += 16 + 8 * n
        else:
            ll, dd = _FIXED
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
                if s > 256:
                    b.pos += 0 if s < 265 or s == 285 else (s - 261) // 4
                    d = b.sym(dd)
                    b.pos += max(0, d // 2 - 1)
        if last:
            return out


# ---- the streams of the issue's table, made once ------------------------------------------------------------------------------------
_CACHE = {}


def _data():
    if "data" not in _CACHE:
        _CACHE["data"] = _text(150000, 9)
    return _CACHE["data"]


def _raw(level, mem):
    """(raw stream, bit offsets of its dynamic blocks behind the first block)"""
    if (level, mem) not in _CACHE:
        raw = _zlib_stream(_data(), 0, [], level=level, mem=mem)
        blocks = _walk(raw)
        _CACHE[(level, mem)] = (raw, [at for at, typ in blocks[1:] if typ == 2], blocks)
    return _CACHE[(level, mem)][:2]


def _stream(level, mem, wrap):
    """(stream in the wrapper, the exact proposals: 8 * header end, then every later dynamic block)"""
    raw, dyn = _raw(level, mem)
    s = _zlib_stream(_data(), wrap, [], level=level, mem=mem)
    h = HEADER[wrap]
    assert s[h:h + len(raw)] == raw
    return s, [8 * h] + [8 * h + at for at in dyn]


def _thin(cuts, gap):
    out = [cuts[0]]
    for c in cuts[1:]:
        if c >= out[-1] + 8 * gap:
            out.append(c)
    return out


def test_walker_agrees_with_the_table():
    """the streams are those the scan was checked on: sizes and block counts of the raw streams"""
    want = {(6, 4): (54822, 28, 22, 0), (6, 2): (57541, 106, 84, 5), (6, 1): (59556, 140, 121, 86), (1, 4): (58241, 31, 27, 0)}
    for (level, mem), (size, dyn, odd, fixed) in want.items():
        _raw(level, mem)
        raw, _, blocks = _CACHE[(level, mem)]
        got = (len(raw), sum(1 for _, t in blocks if t == 2), sum(1 for at, t in blocks if t == 2 and at & 7), sum(1 for _, t in blocks if t == 1))
        assert got == (size, dyn, odd, fixed), ((level, mem), got)


# ---- 1. proposals are exact -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_proposals_are_exact(ctx, wrap, cfg):
    s, want = _stream(cfg[0], cfg[1], wrap)
    got = ctx.find_blocks(s, wrap, 1)
    assert got == want
    assert all(a < b for a, b in zip(got, got[1:]))
    for gap in (1000, 4096):
        assert ctx.find_blocks(s, wrap, gap) == _thin(want, gap)
    assert ctx.find_blocks(s, wrap, 0) == want        # min_gap 0 counts as 1
    cap = len(want) // 2
    assert ctx.find_blocks(s, wrap, 1, cap) == want[:cap]   # (*d_n_cuts == cap: _find reads that many entries)
    assert ctx.find_blocks(s, wrap, 1, 1) == want[:1]
    assert ctx.find_blocks(s, wrap, 1, 0) == []
    assert ctx.find_blocks(s, wrap, 1) == got             # the same entries on every run


def test_auto_wrap_and_empty_input(ctx):
    for wrap in (1, 2):
        s, want = _stream(6, 4, wrap)
        assert ctx.find_blocks(s, 3, 1) == want
    assert ctx.find_blocks(b"", 0, 1) == [0]
    s = zlib.compress(b"")
    assert ctx.find_blocks(s, 1, 1) == [16]
    st, det, olen, used, out, _ = ctx.inflate_bits(s, 1, [16], 4096, 16)
    assert (st, det, olen, used) == (0, 0, 0, len(s))


# ---- 2. round trips through the proposals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 1, 2, 3])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_round_trip_through_proposals(ctx, wrap, cfg):
    data = _data()
    for w in ((1, 2) if wrap == 3 else (wrap,)):
        s, _ = _stream(cfg[0], cfg[1], w)
        for gap in (1, 1000, 4096):
            cuts = ctx.find_blocks(s, wrap, gap)
            st, det, olen, used, out, canary = ctx.inflate_bits(s, wrap, cuts, POM, len(data) + 7)
            assert (st, det) == (0, 0) and olen == len(data) and out == data and used == len(s) and canary, (w, gap, st, det)


@pytest.mark.parametrize("kind", ["random", "run"])
def test_round_trip_whatever_the_scan_proposes(ctx, kind):
    rnd = random.Random(2)
    n = 120000
    data = bytes(rnd.getrandbits(8) for _ in range(n)) if kind == "random" else b"a" * n
    for wrap in (0, 2):
        s = _zlib_stream(data, wrap, [])
        cuts = ctx.find_blocks(s, wrap, 1)
        assert cuts[0] == 8 * HEADER[wrap]
        st, det, olen, used, out, canary = ctx.inflate_bits(s, wrap, cuts, POM, n + 7)
        assert (st, det) == (0, 0) and out == data and used == len(s) and canary, (st, det, len(cuts))


# ---- 3. byte cuts as bit cuts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, INDEPENDENT])
def test_byte_cuts_as_bit_cuts(ctx, flags):
    data = _text(100000, 21 + flags)
    s, c = ctx.deflate(data, 8192, 2, flags)
    b8 = [8 * x for x in c]
    a, b = ctx.inflate(s, 2, c, 8192, len(data) + 7), ctx.inflate_bits(s, 2, b8, 8192, len(data) + 7)
    assert a == b and a[0] == 0 and a[4] == data
    bad = bytearray(s)
    bad[-6] ^= 0x10   # the CRC-32 of the trailer
    a, b = ctx.inflate(bytes(bad), 2, c, 8192, len(data)), ctx.inflate_bits(bytes(bad), 2, b8, 8192, len(data))
    assert a == b and a[:2] == (Z_DATA_ERROR, SI_CHECK)
    for k in (1, 5, len(c) - 1):
        off = list(c)
        off[k] += 1
        a, b = ctx.inflate(s, 2, off, 8192, len(data)), ctx.inflate_bits(s, 2, [8 * x for x in off], 8192, len(data))
        assert a == b and a[0] != 0 and a[1] & 0xFF == SI_CUT
    # cuts that do not ascend, and a cut at the end of the input
    for off in (c[:3] + [c[2]] + c[3:], c[:3] + [c[1]] + c[3:], c + [len(s)]):
        a, b = ctx.inflate(s, 2, off, 8192, len(data)), ctx.inflate_bits(s, 2, [8 * x for x in off], 8192, len(data))
        assert a == b and a[0] != 0 and a[1] & 0xFF == SI_CUT


# ---- 4. mixed proposals ------------------------------------------------------------------------------------------------------------------------
def test_mixed_proposals(ctx):
    data = _data()
    rnd = random.Random(4)
    s = _zlib_stream(data, 2, [rnd.randrange(1, len(data)) for _ in range(12)], mem=4)
    marks = [8 * m for m in ctx.find_cuts(s, 2)]
    assert len(marks) > 8
    for gap in (1, 4096):
        blocks = ctx.find_blocks(s, 2, gap)
        assert len(blocks) > 8
        cuts = sorted(set(marks + blocks))
        if gap == 4096:   # proposals of either kind alone in the list (behind a flush the next block is dynamic: at gap 1 the scan finds it too)
            assert set(marks) - set(blocks) and set(blocks) - set(marks)
        st, det, olen, used, out, canary = ctx.inflate_bits(s, 2, cuts, POM, len(data) + 7)
        assert (st, det) == (0, 0) and out == data and used == len(s) and canary, (gap, st, det)


# ---- 5. a cut off by one bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 2])
def test_cut_off_by_one_bit(ctx, wrap):
    data = _data()
    s, cuts = _stream(6, 4, wrap)
    for k in (1, 8, len(cuts) - 1):
        for d in (1, -1):
            bad = list(cuts)
            bad[k] += d
            st, det, olen, used, out, canary = ctx.inflate_bits(s, wrap, bad, POM, len(data) + 7)
            assert st != 0 and det & 0xFF == SI_CUT and det >> 8 == k and canary, (k, d, st, det)
            st, det, olen, used, out, canary = ctx.inflate_bits(s, wrap, bad[:k] + bad[k + 1:], POM, len(data) + 7)
            assert (st, det) == (0, 0) and out == data and used == len(s)


# ---- 6. false proposals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 2])
def test_false_proposals_inside_a_stored_block(ctx, wrap):
    inner, _ = _raw(6, 4)
    assert len(inner) == 54822
    s = _zlib_stream(inner, wrap, [], level=0)
    cuts = ctx.find_blocks(s, wrap, 1)
    assert len(cuts) >= 20
    calls, first = 0, None
    for _ in range(len(cuts) + 2):
        st, det, olen, used, out, canary = ctx.inflate_bits(s, wrap, cuts, POM, len(inner) + 7)
        calls += 1
        first = first or (st, det & 0xFF)
        assert canary and (st != 0 or out == inner)
        if st == 0:
            break
        assert st == Z_DATA_ERROR and det & 0xFF == SI_CUT and 0 < det >> 8 < len(cuts), (st, det)
        cuts = cuts[:det >> 8] + cuts[(det >> 8) + 1:]
    assert first == (Z_DATA_ERROR, SI_CUT)
    assert st == 0 and out == inner and used == len(s) and calls > 1


# ---- 7. errors and limits ----------------------------------------------------------------------------------------------------------------------------
def test_truncated(ctx):
    data = _data()
    s, cuts = _stream(6, 4, 2)
    for end in (len(s) - 3, len(s) - 8, len(s) // 2):
        t = s[:end]
        st, det, *_ = ctx.inflate_bits(t, 2, [c for c in cuts if c < 8 * end - 64], POM, len(data))
        assert st == Z_BUF_ERROR and det & 0xFF == SI_TRUNC, (end, st, det)


def test_flipped_bit_in_a_middle_piece(ctx):
    data = _data()
    s, cuts = _stream(6, 4, 1)
    for k in range(8):
        b = bytearray(s)
        b[((cuts[10] + cuts[11]) // 2 >> 3) + k] ^= 1 << k
        st, det, olen, used, out, canary = ctx.inflate_bits(bytes(b), 1, cuts, POM, len(data))
        assert st != 0 and canary, (k, st, det)


def test_piece_limit(ctx):
    data = _data()
    s, cuts = _stream(6, 4, 0)
    thin = _thin(cuts, 4096)
    st, det, *_ = ctx.inflate_bits(s, 0, thin, 8192, len(data))
    assert st == Z_BUF_ERROR and det & 0xFF == SI_PIECE and det >> 8 == 0
    # only the last piece is too large: its index is reported
    st, det, *_ = ctx.inflate_bits(s, 0, cuts[:6], 1 << 15, len(data))
    assert st == Z_BUF_ERROR and det & 0xFF == SI_PIECE and det >> 8 == 5


def test_out_cap_one_short(ctx):
    data = _data()
    s, cuts = _stream(6, 2, 2)
    st, det, olen, used, out, canary = ctx.inflate_bits(s, 2, cuts, POM, len(data) - 1)
    assert (st, det, olen) == (Z_BUF_ERROR, SI_OUT, len(data)) and canary and out == data[:-1]


def test_first_cut_must_be_the_header_end(ctx):
    data = _data()
    s, cuts = _stream(6, 4, 2)
    for c0 in (HEADER[2], 8 * HEADER[2] + 1, 0):
        st, det, *_ = ctx.inflate_bits(s, 2, [c0] + cuts[1:], POM, len(data))
        assert st == Z_DATA_ERROR and det & 0xFF == SI_CUT, (c0, st, det)


# ---- 8. launch groups, scratch limit, scan window --------------------------------------------------------------------------------------------------
def _digest(e, pom):
    s, want = _stream(6, 2, 2)
    cuts = e.find_blocks(s, 2, 1)
    assert cuts == want
    r = e.inflate_bits(s, 2, cuts, pom, len(_data()) + 7)
    bad = bytearray(s)
    bad[cuts[50] // 8 + 3] ^= 4
    r2 = e.inflate_bits(bytes(bad), 2, cuts, pom, len(_data()) + 7)
    return r[:4] + (hashlib.sha256(r[4]).hexdigest(), r[5]) + r2[:3]


def test_groups_scratch_limit_and_window_do_not_matter(lib, ctx):
    base = _digest(ctx, 1 << 20)
    assert base[:2] == (0, 0) and base[2] == len(_data()) and base[6] != 0
    e = _Ctx(lib)
    e.ok(lib.zmi_ctx_set_scratch_limit(e.ctx, 64 << 20), "limit")
    assert _digest(e, 1 << 20) == base          # 64 MiB of scratch hold 19 regions of 1 MiB: six launch groups
    e.close()
    code = (
        "import sys, ctypes as C; sys.path.insert(0, %r); import test_emu_stream_inflate_blocks as T\n"
        "e = T._Ctx(T._bind(C.CDLL(T.EMU)))\n"
        "print('digest', repr(T._digest(e, 1 << 20)))\n" % os.path.join(ROOT, "tests"))
    for knobs in ({"ZMI_STREAM_GROUP": "7"}, {"ZMI_BLOCKS_WINDOW": "6000"}):
        r = subprocess.run(["python", "-c", code], env=dict(os.environ, ZMI_TUNING="1", **knobs), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "digest " + repr(base) in r.stdout, (knobs, r.stdout[-500:], r.stderr[-2000:])
