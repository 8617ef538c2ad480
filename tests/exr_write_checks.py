"""Checks of the OpenEXR writer (zmi_exr_bound / zmi_exr_write_dev, include/zmi355.h), shared by tests/test_exr_write_craft.py (CPU, no
library: the judges against each other), tests/test_emu_exr_write.py (CPU, the emulator build) and tests/test_gpu_exr_write.py (the
MI355X), the last two through the C ABI on buffers a `mem` object owns (put / full / read / stream, as in tests/exr_checks.py).

No OpenEXR library stands behind these tests.  The judges, none of them the code under test:
  (a) exr_checks.read_exr parses every written file: channels, windows, the tiled flag and every plane equal the input;
  (b) expected(): the whole expected file from the crafter exr_checks.Exr with injected streams, byte for byte at the levels of
      png_write_checks.EXACT -- every chunk's stream is zlib_header + the payload of the existing zmi_deflate_pieces_dev on
      zip_forward(raw) alone + Adler-32 from zlib, or the raw bytes where that is not shorter than n;
  (c) the library's reader: zmi_exr_headers_dev of the written batch gives status 0 and the records of d_written / d_written_channels,
      byte for byte, zmi_exr_read_dev returns the input regions;
  (d) chunks(): the file's table and chunk headers taken apart with struct -- d_chunk_len is their dataSize, and a chunk with dataSize
      == n holds its raw bytes;
  (e) the fill bytes in front of d_out, behind out_cap and in the alignment gaps, and the canaries behind every table."""
import ctypes as C
import struct
import types
import zlib

import numpy as np

import exr_checks as X
import png_write_checks as PW
from exr_checks import E_ARG, Z_BUF_ERROR, UINT, HALF, FLOAT, NONE, ZIPS, ZIP, ONE_HALF, RGBA, MIXED, LAYOUTS, IMAGE, CHANNEL, Exr
from png_write_checks import EXACT, GUARD, FILL, CANARY, expected_offsets, zlib_header

Z_MEM, E_NOMEM = -4, -102
WORD = int.from_bytes(bytes([CANARY]) * 8, "little")


class WChannel(C.Structure):
    _fields_ = [("name", C.c_char_p), ("pixel_type", C.c_int32)]


class Write(C.Structure):
    """zmi_exr_write (include/zmi355.h)"""
    _fields_ = [("data_window", C.c_int32 * 4), ("display_window", C.c_int32 * 4), ("n_channels", C.c_uint32), ("channels", C.POINTER(WChannel)),
                ("compression", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("flags", C.c_uint32), ("piece_bytes", C.c_uint32),
                ("out_align", C.c_uint32), ("level", C.c_int32), ("strategy", C.c_int32)]


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    X.bind(L)
    PW.bind(L)
    L.zmi_exr_zip_trip.restype, L.zmi_exr_zip_trip.argtypes = u32, []
    L.zmi_exr_bound.restype, L.zmi_exr_bound.argtypes = u64, [vp, u32]
    L.zmi_exr_write_dev.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    return L


def describe(p, pb=4096, level=6, strategy=0, align=1, **over):
    """the zmi_exr_write of the layout of the crafted file p (and what keeps its channel array alive); over: fields set afterwards,
    `channels` as ((name bytes or None, type), ..)"""
    chans = over.pop("channels", tuple((n.encode(), t) for n, t in p.channels))
    arr = (WChannel * max(1, len(chans)))(*[WChannel(n, t) for n, t in chans])
    w = Write((C.c_int32 * 4)(*p.window), (C.c_int32 * 4)(*p.display), len(chans), arr, p.comp, p.tile[0] if p.tile else 0,
              p.tile[1] if p.tile else 0, 0, pb, align, level, strategy)
    for k, v in over.items():
        if k in ("data_window", "display_window"):
            v = (C.c_int32 * 4)(*v)
        setattr(w, k, v)
    return w, arr


def chunks(blob, p):
    """judge (d): [(dataSize, data)] of every chunk of the file in table order, its table and headers checked on the way; the chunks
    must stand densely behind the table and end the file"""
    at = p.table_pos + 8 * p.n_chunks
    out = []
    for k, (x0, y0, w, h) in enumerate(p.boxes):
        assert struct.unpack_from("<Q", blob, p.table_pos + 8 * k)[0] == at, (k, at)
        if p.tile:
            tx, ty, lx, ly, size = struct.unpack_from("<5i", blob, at)
            assert (tx, ty, lx, ly) == (x0 // p.tile[0], y0 // p.tile[1], 0, 0), k
            at += 20
        else:
            y, size = struct.unpack_from("<2i", blob, at)
            assert y == p.ymin + y0, k
            at += 8
        assert 0 < size <= len(p.raw[k]), (k, size)
        out.append((size, blob[at:at + size]))
        at += size
    assert at == len(blob), (at, len(blob))
    return out


class Res:
    def __init__(self, rc, off=None, length=None, status=None, chunk_len=None, written=None, wch=None, out=None, cap=0, guard_ok=True):
        self.rc, self.off, self.len, self.status, self.chunk_len, self.written, self.wch = rc, off, length, status, chunk_len, written, wch
        self.out, self.cap, self.guard_ok = out, cap, guard_ok

    def file(self, i):
        return self.out[self.off[i]:self.off[i] + self.len[i]]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.trip = int(self.L.zmi_exr_zip_trip())
        self.pw = PW.Target(L, ctx, mem)
        self.reader = X.Target(L, ctx, mem)

    def bound(self, p, n, **kw):
        w, keep = describe(p, **kw)
        return int(self.L.zmi_exr_bound(C.addressof(w), n))

    def write(self, files, pb=4096, level=6, strategy=0, align=1, shift=0, gap=3, cap=None, count=None, null=None, tables=True, **over):
        """one zmi_exr_write_dev call on the pixels of the crafted files (ONE layout: that of files[0]), their regions one behind the
        other with `gap` bytes of 0xEE between them.  cap None: zmi_exr_bound"""
        m, p, na = self.mem, files[0], len(files)
        n = na if count is None else count
        blob, offs = bytearray(), []
        for k, f in enumerate(files):
            blob += b"\xEE" * (gap + k % 3 if gap else 0)
            offs.append(len(blob))
            blob += f.want
        w, keep = describe(p, pb, level, strategy, align, **over)
        if cap is None:
            cap = int(self.L.zmi_exr_bound(C.addressof(w), na))
        nc, nch = p.n_chunks, len(p.channels)
        h_in = m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift)
        h_off = m.put(np.array(offs + [0], dtype=np.uint64))
        out = m.full(GUARD + cap + GUARD, FILL)
        h_o, h_l, h_s = m.full((na + 2) * 8, CANARY), m.full((na + 1) * 4, CANARY), m.full((na + 1) * 4, CANARY)
        h_c, h_w, h_wc = m.full((na * nc + 1) * 4, CANARY), m.full((na + 1) * 88, CANARY), m.full((na * nch + 1) * 24, CANARY)
        ptr = {"in": h_in.ptr, "off": h_off.ptr, "out": out.ptr + GUARD, "ooff": h_o.ptr, "olen": h_l.ptr, "st": h_s.ptr, "ctx": self.ctx,
               "w": C.addressof(w), "clen": h_c.ptr if tables else None, "wr": h_w.ptr if tables else None, "wch": h_wc.ptr if tables else None}
        if null:
            ptr[null] = None
        rc = self.L.zmi_exr_write_dev(ptr["ctx"], ptr["w"], ptr["in"], ptr["off"], n, ptr["out"], cap, ptr["ooff"], ptr["olen"], ptr["clen"],
                                      ptr["wr"], ptr["wch"], ptr["st"], m.stream)
        buf = m.read(out, np.uint8)
        if rc != 0:
            untouched = all(bytes(m.read(h, np.uint8)) == bytes([CANARY]) * len(m.read(h, np.uint8)) for h in (h_o, h_l, h_s, h_c, h_w, h_wc))
            return Res(rc, guard_ok=bool((buf == FILL).all()) and untouched)
        off = [int(x) for x in m.read(h_o, np.uint64)]
        if n == 0:
            return Res(0, off[:1], [], [], guard_ok=off[1] == WORD and bool((buf == FILL).all()))
        ln, st = [int(x) for x in m.read(h_l, np.uint32)], [int(x) for x in m.read(h_s, np.int32)]
        cl, wr, wc = m.read(h_c, np.uint32), m.read(h_w, IMAGE), m.read(h_wc, CHANNEL)
        assert off[n + 1] == WORD and ln[n] == WORD & 0xFFFFFFFF and st[n] == WORD & 0xFFFFFFFF, "the call wrote behind its tables"
        assert cl[n * nc:].tobytes() == bytes([CANARY]) * 4 and wr[n:].tobytes() == bytes([CANARY]) * 88, "the call wrote behind its tables"
        assert wc[n * nch:].tobytes() == bytes([CANARY]) * 24, "the call wrote behind its tables"
        if not tables:
            assert (cl.tobytes(), wr.tobytes(), wc.tobytes()) == tuple(bytes([CANARY]) * len(x.tobytes()) for x in (cl, wr, wc))
        body = buf[GUARD:GUARD + cap]
        # nothing outside the files that are complete; a file that crosses out_cap may have left bytes in front of it
        touched = np.zeros(cap, dtype=bool)
        for i in range(n):
            if st[i] == 0:
                touched[off[i]:off[i] + ln[i]] = True
            elif st[i] == Z_BUF_ERROR:
                touched[min(off[i], cap):min(off[i + 1], cap)] = True
        ok = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all() and (body[~touched] == FILL).all())
        return Res(0, off[:n + 1], ln[:n], st[:n], cl[:n * nc].reshape(n, nc), wr[:n], wc[:n * nch].reshape(n, nch), body.tobytes(), cap, ok)

    def expected(self, p, pb, level, strategy):
        """judge (b): the file of the crafter around streams made by the deflate-pieces call alone"""
        stream = {}
        for k, raw in enumerate(p.raw):
            data = raw
            if p.comp != NONE:
                d = X.zip_forward_fast(raw) if len(raw) > 4096 else X.zip_forward(raw)
                cand = zlib_header(level, strategy) + self.pw.payload(d, pb, level, strategy) + struct.pack(">I", zlib.adler32(d))
                if len(cand) < len(raw):
                    data = cand
            stream[k] = data
        return Exr(p.width, p.height, p.channels, p.comp, xmin=p.xmin, ymin=p.ymin, tile=p.tile, planes=p.planes, display=p.display,
                   long_names=any(len(n) > 31 for n, _ in p.channels), stream=stream)


def check(t, r, files, pb=4096, level=6, strategy=0, align=1, exact=None, reader=True, exact_files=None, exact_chunks=None):
    """every judge on a call that had room for all its files; -> the chunks that were stored raw, per file.  Judge (b) costs one
    deflate call per chunk: exact_files / exact_chunks keep it to the first files and to files of at most that many chunks"""
    assert r.rc == 0 and r.guard_ok, (r.rc, r.guard_ok)
    n, p0 = len(files), files[0]
    assert r.status == [0] * n, r.status
    assert r.off == expected_offsets(r.len, align), (r.off[:8], r.len[:8])
    assert r.off[n] <= t.bound(p0, n, pb=pb, level=level, strategy=strategy, align=align)
    exact = level in EXACT if exact is None else exact
    stored = []
    for i, p in enumerate(files):
        blob = r.file(i)
        ref = X.read_exr(blob, FILL)                                              # (a)
        assert ref["channels"] == [(a, b) for a, b in p.channels] and ref["data_window"] == p.window and ref["display_window"] == tuple(p.display)
        assert ref["tiled"] == bool(p.tile) and ref["region"] == p.want, i
        got = chunks(blob, p)                                                     # (d)
        assert [s for s, _ in got] == [int(x) for x in r.chunk_len[i]], i
        for k, (size, data) in enumerate(got):
            assert size < len(p.raw[k]) or data == p.raw[k], (i, k)
            assert p.comp != NONE or size == len(p.raw[k])
        stored.append([s == len(raw) for (s, _), raw in zip(got, p.raw)])
        if exact and (exact_files is None or i < exact_files) and (exact_chunks is None or p.n_chunks <= exact_chunks):   # (b)
            want = t.expected(p, pb, level, strategy)
            assert stored[-1] == want.stored, (i, stored[-1], want.stored)
            if blob != want.blob:
                bad = next(k for k in range(min(len(blob), len(want.blob))) if blob[k] != want.blob[k]) if len(blob) == len(want.blob) else -1
                raise AssertionError("file %d (%d x %d, %s, compression %d, level %d): %d bytes, expected %d, first difference at %d"
                                     % (i, p.width, p.height, p.channels, p.comp, level, len(blob), len(want.blob), bad))
    if reader:                                                                    # (c)
        nch = len(p0.channels)
        b = t.reader.headers([types.SimpleNamespace(blob=r.file(i)) for i in range(n)], shift=3, gap=5, chan_cap=nch)
        assert b.rc == 0 and [int(x) for x in b.rec["status"]] == [0] * n
        assert b.rec.tobytes() == r.written.tobytes() and b.chans.tobytes() == r.wch.tobytes()
        rd = t.reader.read(b, align=4)
        assert rd.rc == 0 and rd.clean and rd.status == [0] * n and rd.detail == [0] * n, (rd.status, rd.detail)
        assert [rd.slot(j) for j in range(n)] == [p.want for p in files]
    return stored


def run(t, files, **kw):
    wkw = {k: kw[k] for k in ("pb", "level", "strategy", "align", "shift") if k in kw}
    r = t.write(files, **wkw)
    ckw = {k: kw[k] for k in ("pb", "level", "strategy", "align", "exact", "reader", "exact_files", "exact_chunks") if k in kw}
    r.stored = check(t, r, files, **ckw)
    return r


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------------------
def geometry(t, widths=(1, 2, 3, 5, 17, 63, 64, 65, 257), heights=(1, 15, 16, 17, 33), comps=(ZIPS, ZIP, NONE), layouts=LAYOUTS):
    """every width x height x compression x channel layout, three images a call: h even and odd, runs shorter than a lane's 32 bytes, a
    short last chunk, planes that start at an odd multiple of 2.  Judge (b) on the first image of the files of at most 3 chunks"""
    n = 0
    for li, layout in enumerate(layouts):
        for comp in comps:
            for h in heights:
                for w in widths:
                    run(t, [Exr(w, h, layout, comp, seed=w + 3 * h + li + 7 * k) for k in range(3)], align=16, shift=li, pb=1024, exact_files=1, exact_chunks=3)
                    n += 1
    return n


def trips(t, comps=(ZIPS, ZIP)):
    """run lengths at a trip's size - 2, + 0, + 2 bytes in HALF pixels and - 4, + 0, + 4 in FLOAT pixels next to a HALF channel (the
    second run then starts at an odd multiple of 2); chunk sizes with h mod 16 in {0, 1, 2, 15}: the seam between the halves and the
    misaligned second stream"""
    T, n = t.trip, 0
    for comp in comps:
        for size in (T - 2, T, T + 2):
            run(t, [Exr(size // 2, 3, ONE_HALF, comp, seed=size)], pb=4096)
            n += 1
        for size in (T - 4, T, T + 4):
            run(t, [Exr(size // 4, 2, (("A", HALF), ("Z", FLOAT)), comp, seed=size + 1)], pb=4096)
            n += 1
    for h_mod, w in ((0, 16), (1, 17), (2, 18), (15, 15)):                        # one row of w HALF pixels: n = 2 w, h = w
        p = Exr(w, 2, ONE_HALF, ZIPS, seed=w)
        assert len(p.raw[0]) // 2 % 16 == h_mod
        run(t, [p, Exr(w, 2, ONE_HALF, ZIPS, seed=w + 1)])
        n += 1
    return n


def tiles(t, sizes=((16, 16), (32, 8))):
    """tiles of 16 x 16 and 32 x 8 on 37 x 21 (all four chunk size classes) and on exactly one tile, ZIP and NONE, windows off the origin"""
    n = 0
    for tw, th in sizes:
        for comp in (ZIP, NONE):
            run(t, [Exr(37, 21, RGBA, comp, tile=(tw, th), seed=tw + comp + k, xmin=-5, ymin=3) for k in range(2)], align=16, pb=512)
            run(t, [Exr(tw, th, MIXED, comp, tile=(tw, th), seed=th + comp, xmin=7, ymin=-9)], pb=512)
            n += 2
    return n


def raw_rule(t):
    """noise chunks among smooth ones: dataSize == n exactly at the noise chunks; level 0: every chunk raw; one HALF pixel under ZIPS
    (n = 2); a file of noise only"""
    a = [Exr(70, 50, RGBA, ZIP, noise=(1, 3), seed=3), Exr(70, 50, RGBA, ZIP, noise=(0,), seed=4)]
    r = run(t, a, pb=1024)
    assert r.stored == [[False, True, False, True], [True, False, False, False]]
    assert [[int(x) == len(raw) for x, raw in zip(r.chunk_len[i], a[i].raw)] for i in range(2)] == r.stored
    b = [Exr(37, 21, ONE_HALF, ZIP, tile=(16, 16), noise=(2, 5), seed=5)]
    assert run(t, b, pb=256).stored == [[False, False, True, False, False, True]]
    c = [Exr(33, 9, MIXED, ZIPS, seed=6)]
    assert run(t, c, level=0).stored == [[True] * 9]
    d = [Exr(1, 3, ONE_HALF, ZIPS, seed=7)]
    assert run(t, d).stored == [[True] * 3] and len(d[0].raw[0]) == 2
    e = [Exr(19, 20, RGBA, ZIP, noise=(0, 1), seed=8)]
    assert run(t, e).stored == [[True, True]]
    return 5


def pieces(t, levels=(1, 6, 9, 0)):
    """piece_bytes of 256 and 4096 on chunks of several pieces (16 x 150 RGBA HALF: 19 200 bytes), the four kinds of level"""
    files, n = [Exr(150, 20, RGBA, ZIP, seed=9), Exr(150, 20, RGBA, ZIP, noise=(1,), seed=10)], 0
    for level in levels:
        for pb in (256, 4096):
            run(t, files, pb=pb, level=level, align=16)
            n += 1
    return n


def across_groups(t, files, pb, groups, set_group, level=6):
    """the same bytes in one launch group and in forced groups of `groups` pieces each"""
    ref = run(t, files, pb=pb, level=level, align=16)
    for g in groups:
        set_group(g)
        try:
            r = t.write(files, pb=pb, level=level, align=16)
        finally:
            set_group(None)
        assert (r.rc, r.off, r.len, r.status, r.out) == (0, ref.off, ref.len, ref.status, ref.out), g
        assert r.chunk_len.tobytes() == ref.chunk_len.tobytes() and r.written.tobytes() == ref.written.tobytes() and r.guard_ok
    return len(groups)


def launch_groups(t, set_group):
    """three files of three chunks of 10, 10 and 5 pieces, one of them noise: groups of one chunk (10 pieces; 7 rounds down to none, so
    one), which end between the chunks of a file, and of two chunks (25), which end inside files and between them"""
    files = [Exr(20, 40, RGBA, ZIP, seed=11), Exr(20, 40, RGBA, ZIP, noise=(1,), seed=12), Exr(20, 40, RGBA, ZIP, seed=13)]
    assert [-(-len(raw) // 256) for raw in files[0].raw] == [10, 10, 5]
    return across_groups(t, files, 256, (10, 7, 25), set_group)


def independence(t, shifts=(0, 1, 3, 15), aligns=(1, 16, 4096)):
    """the input at every shift, an image alone and in another slot of a larger batch, every output alignment: the same file bytes"""
    p = Exr(61, 35, MIXED, ZIP, noise=(1,), seed=14)
    others = [Exr(61, 35, MIXED, ZIP, seed=15 + k) for k in range(4)]
    ref, n = run(t, [p]).file(0), 0
    for shift in shifts:
        assert t.write([p], shift=shift).file(0) == ref
        n += 1
    for align in aligns:
        r = t.write(others[:3] + [p] + others[3:], align=align, shift=align % 7)
        assert r.rc == 0 and r.guard_ok and r.status == [0] * 5 and r.off == expected_offsets(r.len, align) and r.file(3) == ref, align
        n += 1
    return n


def pin(t):
    """the 363-byte example of include/zmi355.h, byte for byte"""
    from test_exr_craft import PIN2, PIN2_G, PIN2_Z
    p = Exr(3, 2, (("G", HALF), ("Z", FLOAT)), NONE, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z])
    r = run(t, [p])
    assert r.file(0) == PIN2 and r.len == [363]
    return 1


def capacity(t, aligns=(1, 16, 4096)):
    """out_cap exact, one byte short, cut behind the second file, and 0: offsets and need unchanged, Z_BUF_ERROR with length 0 from the
    first file that crosses the cap, complete files in front, nothing behind the cap"""
    files, n = [Exr(9, 20, RGBA, ZIP, seed=16), Exr(9, 20, RGBA, ZIP, noise=(0,), seed=17), Exr(9, 20, RGBA, ZIP, seed=18)], 0
    for align in aligns:
        ref = run(t, files, align=align, pb=512)
        ends = [ref.off[i] + ref.len[i] for i in range(3)]
        for cap in (ends[2], ends[2] - 1, ends[1], 0):
            r = t.write(files, align=align, pb=512, cap=cap)
            fits = [e <= cap for e in ends]
            assert r.rc == 0 and r.guard_ok, (align, cap)
            assert r.off == ref.off and r.status == [0 if f else Z_BUF_ERROR for f in fits], (align, cap, r.off, r.status)
            assert r.len == [ln if f else 0 for ln, f in zip(ref.len, fits)] and r.chunk_len.tobytes() == ref.chunk_len.tobytes()
            for i in range(3):
                if fits[i]:
                    assert r.file(i) == ref.file(i) and r.written[i].tobytes() == ref.written[i].tobytes() and r.wch[i].tobytes() == ref.wch[i].tobytes()
                else:
                    z = np.zeros(1, dtype=IMAGE)
                    z[0]["status"] = Z_BUF_ERROR
                    assert r.written[i].tobytes() == z.tobytes() and r.wch[i].tobytes() == bytes(24 * 4)
            n += 1
    return n


def arguments(t):
    """every ZMI_E_ARG the header names as a return value, nothing written; NULL tables; n_images 0; the bound of an invalid layout"""
    p, n = Exr(5, 4, MIXED, ZIP, seed=19), 0
    bad = [dict(data_window=(3, 0, 2, 5)), dict(data_window=(0, 9, 5, 8)), dict(display_window=(1, 0, 0, 0)),
           dict(data_window=(-(1 << 31), 0, (1 << 31) - 1, 0)), dict(data_window=(0, 0, 70000, 70000)),
           dict(data_window=(0, 0, (1 << 30), 0), channels=tuple((b"c%d" % k, FLOAT) for k in range(2))),
           dict(n_channels=0), dict(channels=((b"A", 3), (b"B", HALF))), dict(channels=((b"A", -1),)), dict(channels=((b"", HALF),)),
           dict(channels=((None, HALF),)), dict(channels=((b"x" * 256, HALF),)), dict(channels=((b"B", HALF), (b"A", HALF))),
           dict(channels=((b"A", HALF), (b"A", FLOAT))), dict(channels=((b"a", HALF), (b"Z", HALF))), dict(compression=1), dict(compression=4),
           dict(tile_w=16), dict(tile_h=16), dict(pb=0), dict(pb=(1 << 30) + 1), dict(level=10), dict(level=-2), dict(strategy=5),
           dict(strategy=-1), dict(align=0), dict(align=3), dict(align=8192), dict(flags=1),
           # the region fits 32 bits with 65 535 bytes to spare, the table and the chunk headers of 16 384 scanlines do not
           dict(data_window=(0, 0, 65534, 16383), channels=((b"Z", FLOAT),), compression=ZIPS),
           dict(data_window=(0, 0, 0, 1 << 24), compression=ZIPS, count=200), dict(data_window=(0, 0, 1 << 24, 0), pb=1, count=64)]
    for kw in bad:
        r = t.write([p], cap=64, **kw)
        assert r.rc == E_ARG and r.guard_ok and t.L.zmi_last_error(), kw
        if "count" not in kw:
            assert t.bound(p, 1, **kw) == 0, kw
        n += 1
    for null in ("ctx", "w", "in", "off", "out", "ooff", "olen", "st"):
        assert t.write([p], null=null).rc == E_ARG, null
        n += 1
    r = t.write([p], count=0, cap=0)
    assert (r.rc, r.off, r.guard_ok) == (0, [0], True)
    r = t.write([p], tables=False)
    assert r.rc == 0 and r.guard_ok and r.status == [0] and r.file(0) == run(t, [p]).file(0)
    long = Exr(5, 4, (("a channel with a name of more than 31 bytes", HALF), ("b", FLOAT)), ZIPS, long_names=True, seed=20)
    run(t, [long])
    return n + 3
