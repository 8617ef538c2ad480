"""CPU tests of the single-stream inflate on the device: zmi_inflate_stream_dev and zmi_stream_find_cuts_dev (include/zmi355.h;
csrc/inflate.hip, zmi_api.hip) on the emulator build.  The inverse of zmi_deflate_stream_dev: one raw / zlib / gzip stream whose
pieces start behind flush markers is decoded piece-parallel (symbolic resolve, window scan, substitute) and its wrapper checked.
What is checked: round trips of this library's own streams in both modes and several piece sizes, streams of Python's zlib with
sync / full flushes at random points read through the proposals of find_cuts (a stored block holding the marker included), a gzip
header with every optional field, every error the API names, the canary behind out_cap, and independence of the scratch limit."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libzmi355_emu.so")
WBITS = {0: -15, 1: 15, 2: 31}
INDEPENDENT = 1
Z_DATA_ERROR, Z_BUF_ERROR, Z_NEED_DICT = -3, -5, 2
SI_CUT, SI_PIECE, SI_CHECK, SI_LENGTH, SI_OUT, SI_TRUNC, SI_DICT = 3, 4, 7, 8, 9, 2, 10


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
    L.zmi_stream_find_cuts_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
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

    def find_cuts(self, s, wrap, min_gap=1, cap=4096):
        inp = np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy()
        cuts = np.zeros(cap, dtype=np.uint64)
        cnt = np.zeros(1, dtype=np.uint32)
        self.ok(self.L.zmi_stream_find_cuts_dev(self.ctx, _p(inp), len(s), wrap, min_gap, _p(cuts), cap, _p(cnt), None), "find_cuts")
        return [int(x) for x in cuts[:int(cnt[0])]]

    def inflate(self, s, wrap, cuts, piece_out_max, out_cap):
        """-> (status, detail, out_len, in_used, output bytes, canary intact)"""
        inp = np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy()
        cu = np.array(cuts, dtype=np.uint64)
        out = np.full(out_cap + 256, 0x5A, dtype=np.uint8)
        w = np.zeros(4, dtype=np.uint64)   # out_len | in_used | status, detail (int32)
        self.ok(self.L.zmi_inflate_stream_dev(self.ctx, _p(inp), len(s), wrap, _p(cu), len(cuts), piece_out_max, _p(out), out_cap,
                                              _p(w), _p(w) + 8, _p(w) + 16, _p(w) + 20, None), "zmi_inflate_stream_dev")
        st, det = (int(x) for x in w[2:3].view(np.int32))
        olen = int(w[0])
        return st, det, olen, int(w[1]), bytes(out[:min(olen, out_cap)]), bool((out[out_cap:] == 0x5A).all())


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


def _zlib_stream(data, wrap, points, mode=zlib.Z_SYNC_FLUSH, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap])
    out, at = [], 0
    for p in sorted(points) + [len(data)]:
        out.append(c.compress(data[at:p]))
        if p < len(data):
            out.append(c.flush(mode))
        at = p
    out.append(c.flush())
    return b"".join(out)


@pytest.mark.parametrize("wrap", [0, 1, 2])
@pytest.mark.parametrize("flags", [0, INDEPENDENT])
@pytest.mark.parametrize("piece", [1024, 8192, 20480, 65536, 7777])
def test_round_trip_own_streams(ctx, wrap, flags, piece):
    data = _text(150000, piece + wrap)
    s, idx = ctx.deflate(data, piece, wrap, flags)
    st, det, olen, used, out, canary = ctx.inflate(s, wrap, idx, piece, len(data) + 7)
    assert (st, det) == (0, 0) and olen == len(data) and out == data and used == len(s) and canary


@pytest.mark.parametrize("wrap", [0, 1, 2])
def test_empty_input(ctx, wrap):
    s, idx = ctx.deflate(b"", 4096, wrap)
    st, det, olen, used, out, _ = ctx.inflate(s, wrap, idx, 4096, 16)
    assert (st, olen, used) == (0, 0, len(s))


def test_auto_wrap(ctx):
    data = _text(40000, 3)
    for wrap in (1, 2):
        s, idx = ctx.deflate(data, 8192, wrap)
        st, _, olen, used, out, _ = ctx.inflate(s, 3, idx, 8192, len(data))
        assert st == 0 and out == data and used == len(s)


@pytest.mark.parametrize("kind", ["text", "random", "run"])
@pytest.mark.parametrize("mode", [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])
def test_python_zlib_streams_through_find_cuts(ctx, kind, mode):
    rnd = random.Random({"text": 1, "random": 2, "run": 3}[kind] * 10 + mode)
    n = 120000
    data = {"text": _text(n, 9), "random": bytes(rnd.getrandbits(8) for _ in range(n)), "run": b"\x61" * n}[kind]
    points = [rnd.randrange(1, n) for _ in range(30)]
    for wrap in (0, 2):
        s = _zlib_stream(data, wrap, points, mode)
        cuts = ctx.find_cuts(s, wrap)
        assert len(cuts) > 10
        st, det, olen, used, out, _ = ctx.inflate(s, wrap, cuts, 1 << 17, n)
        assert st == 0 and out == data and used == len(s), (st, det)


def test_run_across_many_small_pieces(ctx):
    """a run of one byte over many pieces shorter than the window: every window is a shifted copy of the one in front"""
    data = b"\x00" * 70000 + b"xyz" + b"\x00" * 30000
    s = _zlib_stream(data, 1, list(range(500, 100000, 997)))
    cuts = ctx.find_cuts(s, 1)
    st, det, olen, used, out, _ = ctx.inflate(s, 1, cuts, 4096, len(data))
    assert st == 0 and out == data and used == len(s), (st, det)


def test_stored_block_holding_the_marker(ctx):
    """level 0 stores the bytes: the 00 00 FF FF inside the data is a false proposal.  Right bytes, or a non-zero status"""
    rnd = random.Random(5)
    data = bytes(rnd.getrandbits(8) for _ in range(3000)) + b"\x00\x00\xff\xff" + bytes(rnd.getrandbits(8) for _ in range(3000))
    s = _zlib_stream(data, 2, [2000, 4500], level=0)
    cuts = ctx.find_cuts(s, 2)
    st, det, olen, used, out, _ = ctx.inflate(s, 2, cuts, 1 << 16, len(data))
    assert st != 0 or out == data
    assert st == Z_DATA_ERROR and det & 0xFF == SI_CUT   # the proposal inside the block cannot verify
    bad = det >> 8
    st, det, olen, used, out, _ = ctx.inflate(s, 2, cuts[:bad] + cuts[bad + 1:], 1 << 16, len(data))
    assert st == 0 and out == data


def test_gzip_header_with_every_field(ctx):
    data = _text(30000, 11)
    raw = _zlib_stream(data, 0, [10000, 20000])
    hdr = bytearray(b"\x1f\x8b\x08\x1e" + b"\x00" * 4 + b"\x00\x03")
    hdr += struct.pack("<H", 5) + b"extra" + b"name.txt\x00" + b"a comment\x00"
    hdr += struct.pack("<H", zlib.crc32(bytes(hdr)) & 0xFFFF)
    s = bytes(hdr) + raw + struct.pack("<II", zlib.crc32(data), len(data))
    cuts = ctx.find_cuts(s, 2)
    assert cuts[0] == len(hdr)
    st, det, olen, used, out, _ = ctx.inflate(s, 2, cuts, 1 << 16, len(data))
    assert st == 0 and out == data and used == len(s)
    bad = bytearray(s)
    bad[len(hdr) - 1] ^= 1   # FHCRC
    st, *_ = ctx.inflate(bytes(bad), 2, cuts, 1 << 16, len(data))
    assert st == Z_DATA_ERROR


def test_trailer_errors(ctx):
    data = _text(50000, 12)
    for wrap, pos, det_want in ((1, -1, SI_CHECK), (2, -5, SI_CHECK), (2, -1, SI_LENGTH)):
        s, idx = ctx.deflate(data, 8192, wrap)
        b = bytearray(s)
        b[pos] ^= 0x10
        st, det, *_ = ctx.inflate(bytes(b), wrap, idx, 8192, len(data))
        assert (st, det) == (Z_DATA_ERROR, det_want)


def test_truncated(ctx):
    data = _text(50000, 13)
    s, idx = ctx.deflate(data, 8192, 2)
    for cut in (len(s) - 3, len(s) - 8, len(s) // 2, 5):
        t = s[:cut]
        st, det, *_ = ctx.inflate(t, 2, [i for i in idx if i < cut] or [10], 8192, len(data))
        assert st == Z_BUF_ERROR, (cut, st, det)


def test_flipped_bit_in_a_middle_piece(ctx):
    data = _text(80000, 14)
    s, idx = ctx.deflate(data, 8192, 1)
    for k in range(8):
        b = bytearray(s)
        p = (idx[4] + idx[5]) // 2 + k
        b[p] ^= 1 << k
        st, det, olen, used, out, _ = ctx.inflate(bytes(b), 1, idx, 8192, len(data))
        assert st != 0 or out == data


def test_index_off_by_one(ctx):
    data = _text(80000, 15)
    s, idx = ctx.deflate(data, 8192, 2)
    for d in (-1, 1):
        bad = list(idx)
        bad[3] += d
        st, det, *_ = ctx.inflate(s, 2, bad, 8192, len(data))
        assert st != 0 and det & 0xFF == SI_CUT, (st, det)


def test_piece_limit(ctx):
    data = _text(80000, 16)
    s, idx = ctx.deflate(data, 16384, 0)
    st, det, *_ = ctx.inflate(s, 0, idx, 8192, len(data))
    assert st != 0 and det & 0xFF == SI_PIECE


def test_out_cap_one_short(ctx):
    data = _text(50000, 17)
    s, idx = ctx.deflate(data, 8192, 2)
    st, det, olen, used, out, canary = ctx.inflate(s, 2, idx, 8192, len(data) - 1)
    assert (st, det, olen) == (Z_BUF_ERROR, SI_OUT, len(data)) and canary and out == data[:-1]


def test_fdict(ctx):
    s = bytes([0x78, 0xBB]) + b"\x00\x00\x00\x01" + zlib.compress(b"abc")[2:]
    assert (0x78 * 256 + 0xBB) % 31 == 0
    st, det, *_ = ctx.inflate(s, 1, [2], 4096, 16)
    assert (st, det) == (Z_NEED_DICT, SI_DICT)


def test_distance_before_the_stream(ctx):
    """a piece whose first match reaches in front of the stream's start"""
    # raw: piece 0 = the stored bytes "ab", piece 1 = a fixed block with a match of distance 3 (one byte too far)
    p0 = b"\x00\x02\x00\xfd\xffab" + b"\x00\x00\x00\xff\xff"
    bits, nb = 0, 0

    def put(v, n):
        nonlocal bits, nb
        bits |= v << nb
        nb += n

    def rev(v, n):
        return int(format(v, "0%db" % n)[::-1], 2)
    put(1, 1); put(1, 2)                 # BFINAL, fixed
    put(rev(0b0000001, 7), 7)            # length 3 (code 257)
    put(rev(2, 5), 5)                    # distance 3
    put(rev(0, 7), 7)                    # end of block
    p1 = bits.to_bytes((nb + 7) // 8, "little")
    s = p0 + p1
    st, det, *_ = ctx.inflate(s, 0, [0, len(p0)], 4096, 64)
    assert st == Z_DATA_ERROR
    st, det, olen, used, out, _ = ctx.inflate(b"\x00\x03\x00\xfc\xffabc" + b"\x00\x00\x00\xff\xff" + p1, 0, [0, 13], 4096, 64)
    assert st == 0 and out == b"abcabc"


def test_scratch_limit_does_not_matter(lib):
    data = _text(600000, 18)
    res = []
    for limit in (None, 64 << 20):
        e = _Ctx(lib)
        if limit:
            e.ok(lib.zmi_ctx_set_scratch_limit(e.ctx, limit), "limit")
        s, idx = e.deflate(data, 4096, 2)
        res.append(e.inflate(s, 2, idx, 4096, len(data)))
        b = bytearray(s)
        b[idx[100] + 3] ^= 4
        res.append(e.inflate(bytes(b), 2, idx, 4096, len(data))[:3])
        e.close()
    assert res[0][0] == 0 and res[0][4] == data
    assert res[0] == res[2] and res[1] == res[3]


def test_several_launch_groups(lib, monkeypatch):
    """the group size from ZMI_STREAM_GROUP (a tuning knob read only with ZMI_TUNING): offsets and windows chain across groups"""
    data = _text(200000, 19)
    code = (
        "import sys, ctypes as C; sys.path.insert(0, %r); import test_emu_stream_inflate as T\n"
        "L = T._bind(C.CDLL(T.EMU)); e = T._Ctx(L); d = T._text(200000, 19)\n"
        "for flags in (0, 1):\n"
        "    s, idx = e.deflate(d, 3000, 2, flags)\n"
        "    r = e.inflate(s, 2, idx, 3000, len(d))\n"
        "    assert r[0] == 0 and r[4] == d, r[:4]\n"
        "print('ok')\n" % os.path.join(ROOT, "tests"))
    env = dict(os.environ, ZMI_TUNING="1", ZMI_STREAM_GROUP="7")
    r = subprocess.run(["python", "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    assert len(data) == 200000
