"""Checks of the TIFF writer (zmi_tiff_write_dev, include/zmi355.h), shared by tests/test_tiff_write_craft.py (CPU, no library: the
judges against each other and against PIL), tests/test_emu_tiff_write.py (CPU, the emulator build) and tests/test_gpu_tiff_write.py
(the MI355X), the last two through the C ABI on buffers a `mem` object owns (put / full / read / stream, as in tests/tiff_checks.py).

The judges, none of them the code under test:
  (a) parse(): the file taken apart with struct -- header, the one IFD, every value --, zlib.decompress of every segment, then
      tiff_checks.unpredict: the samples must be the input's, the geometry tags what *w says;
  (b) craft(): the whole expected file from struct.pack after the layout the header states; every segment's stream is the zlib header,
      the pieces of tiff_checks.predict(...) through the existing zmi_deflate_pieces_dev alone (png_write_checks.Target.payload) and
      zlib.adler32 -- compared byte for byte, gap bytes included, at the levels of png_write_checks.EXACT;
  (c) PIL, where it imports with libtiff, for the formats it reads: uint8 gray / RGB / RGBA, uint16 gray, float32 gray -- an extra judge,
      never the only one;
  (d) the library's reader: zmi_tiff_directory_dev of the written file gives status 0 and the record d_written holds, byte for byte;
      zmi_tiff_read_dev in both modes returns the input;
  (e) guards: the fill bytes in front of d_out and behind out_cap, the canaries behind every table."""
import ctypes as C
import io
import struct
import types
import zlib

import numpy as np

import png_write_checks as PW
import tiff_checks as TC
from png_write_checks import EXACT, zlib_header
from tiff_checks import predict, unpredict, samples_of, PAGE, E_ARG, Z_BUF_ERROR, ASSEMBLE, SHIFTS, SHORT, LONG, LONG8

BIGTIFF = 2
GUARD, FILL, CANARY = 64, 0xC7, 0x77
SCAN_MAX = 0x7F000000

try:
    from PIL import Image, features
    HAVE_PIL = bool(features.check("libtiff"))
except ImportError:                                          # judge (c) is then left out
    Image, HAVE_PIL = None, False


class Write(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("rows_per_strip", C.c_uint32),
                ("bits", C.c_uint16), ("samples", C.c_uint16), ("sample_format", C.c_uint16), ("predictor", C.c_uint16),
                ("photometric", C.c_uint16), ("extra_samples", C.c_uint16), ("extra_kind", C.c_uint16), ("flags", C.c_uint32),
                ("piece_bytes", C.c_uint32), ("out_align", C.c_uint32), ("level", C.c_int32), ("strategy", C.c_int32)]


assert C.sizeof(Write) == 56


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    TC.bind(L)
    L.zmi_tiff_predict_tile.restype = u32
    L.zmi_tiff_predict_tile.argtypes = []
    L.zmi_tiff_bound.restype = u64
    L.zmi_tiff_bound.argtypes = [vp]
    L.zmi_tiff_write_dev.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    return L


# ---- the pages ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One page to write.  tile = (tile_w, tile_h) or None for strips of rps rows (0 / None: one strip).  `image` = the [H, W, C] bytes,
    `segs[k]` = the dense region of segment k with noise in the padding of edge tiles, `segs_zero[k]` = the same with zeros there (what
    assemble mode makes).  Full-range samples, so every difference of predictor 2 wraps."""

    def __init__(self, width, height, samples=1, bits=8, fmt=1, pred=1, tile=None, rps=None, big=False, extra=0, extra_kind=2,
                 photometric=None, seed=1):
        self.width, self.height, self.samples, self.bits, self.fmt, self.pred = width, height, samples, bits, fmt, pred
        self.tile, self.rps, self.big, self.extra, self.extra_kind = tile, rps, big, extra, extra_kind
        self.photometric = photometric if photometric is not None else (2 if samples >= 3 else 1)
        self.sb = sb = bits // 8
        self.pb = samples * sb
        self.seg_w, self.seg_h = tile if tile else (width, height if not rps or rps >= height else rps)
        self.across, self.down = -(-width // self.seg_w), -(-height // self.seg_h)
        self.n_segs = self.across * self.down
        ch, cw = (self.down * self.seg_h, self.across * self.seg_w) if tile else (height, width)
        canvas = np.frombuffer(samples_of(ch * cw * samples, sb, seed), dtype=np.uint8).reshape(ch, cw, self.pb)
        zero = np.zeros_like(canvas)
        zero[:height, :width] = canvas[:height, :width]
        self.image = np.ascontiguousarray(canvas[:height, :width]).tobytes()
        self.segs, self.segs_zero, self.rows = [], [], []
        for k in range(self.n_segs):
            ty, tx = divmod(k, self.across)
            rows = self.seg_h if tile else min(self.seg_h, height - ty * self.seg_h)
            for src, dst in ((canvas, self.segs), (zero, self.segs_zero)):
                dst.append(np.ascontiguousarray(src[ty * self.seg_h:ty * self.seg_h + rows, tx * self.seg_w:(tx + 1) * self.seg_w]).tobytes())
            self.rows.append(rows)

    def desc(self, assemble=False, pb=4096, level=6, strategy=0, align=16, **over):
        w = Write(self.width, self.height, self.tile[0] if self.tile else 0, self.tile[1] if self.tile else 0, self.rps or 0, self.bits,
                  self.samples, self.fmt, self.pred, self.photometric, self.extra, self.extra_kind,
                  (ASSEMBLE if assemble else 0) | (BIGTIFF if self.big else 0), pb, align, level, strategy)
        for name, v in over.items():
            setattr(w, name, v)
        return w

    def predicted(self, segs, k):
        """what the compressor of segment k is handed (tiff_checks.predict, checked against its unpredict)"""
        raw = predict(segs[k], self.rows[k], self.seg_w, self.samples, self.sb, self.pred, False)
        assert unpredict(raw, self.rows[k], self.seg_w, self.samples, self.sb, self.pred, False) == segs[k]
        return raw


# ---- judge (b): the crafter -----------------------------------------------------------------------------------------------------------------
def entries(c):
    """(tag, type, values) ascending by tag; the values of the two arrays are None"""
    seg_t = LONG8 if c.big else LONG
    ent = [(256, LONG, [c.width]), (257, LONG, [c.height]), (258, SHORT, [c.bits] * c.samples), (259, SHORT, [8]), (262, SHORT, [c.photometric]),
           (277, SHORT, [c.samples]), (284, SHORT, [1]), (317, SHORT, [c.pred]), (339, SHORT, [c.fmt] * c.samples)]
    if c.extra:
        ent.append((338, SHORT, [c.extra_kind] * c.extra))
    if c.tile:
        ent += [(322, LONG, [c.seg_w]), (323, LONG, [c.seg_h]), (324, seg_t, None), (325, seg_t, None)]
    else:
        ent += [(273, seg_t, None), (278, LONG, [c.seg_h]), (279, seg_t, None)]
    return sorted(ent)


def craft(c, streams, align):
    """the file the header's layout describes around given segment streams"""
    big = c.big
    os_, es, cs, ifd = (8, 20, 8, 16) if big else (4, 12, 2, 8)
    ent = entries(c)
    at = ifd + cs + len(ent) * es + os_                                     # where the out-of-line values start
    where, sizes = {}, {}
    for tag, typ, vals in ent:
        n = c.n_segs if vals is None else len(vals)
        sizes[tag] = n * TC.TYPE_SIZE[typ]
        if sizes[tag] > os_:
            at += at % 2
            where[tag] = at
            at += sizes[tag]
    offs, cnts, p = [], [], at
    for s in streams:
        p = -(-p // align) * align
        offs.append(p)
        cnts.append(len(s))
        p += len(s)
    out = bytearray(p)
    out[:ifd] = b"II" + (struct.pack("<HHHQ", 43, 8, 0, 16) if big else struct.pack("<HI", 42, 8))
    struct.pack_into("<Q" if big else "<H", out, ifd, len(ent))
    for q, (tag, typ, vals) in enumerate(ent):
        ea = ifd + cs + q * es
        if vals is None:
            vals = offs if tag in (273, 324) else cnts
        raw = struct.pack("<%d%s" % (len(vals), TC.TYPE_FMT[typ]), *vals)
        struct.pack_into("<HHQ" if big else "<HHI", out, ea, tag, typ, len(vals))
        if tag in where:
            struct.pack_into("<Q" if big else "<I", out, ea + 4 + os_, where[tag])
            out[where[tag]:where[tag] + len(raw)] = raw
        else:
            out[ea + 4 + os_:ea + 4 + os_ + len(raw)] = raw
    for o, s in zip(offs, streams):
        out[o:o + len(s)] = s
    return bytes(out)


def host_streams(c, segs, level=6):
    """segment streams from the host's zlib: what the craft tests hand to craft()"""
    return [zlib.compress(c.predicted(segs, k), level) for k in range(c.n_segs)]


# ---- judge (a): the parser ------------------------------------------------------------------------------------------------------------------
def parse(file, strict=True):
    """-> (tags, segs): tags = {tag: (type, [values], the file position of the values)}, segs = the decoded segments, predictor undone,
    little-endian.  strict: the file is one of this writer's -- little-endian, one IFD right behind the header, tags ascending and each
    of them once, the next-IFD offset 0, the file ending with the last segment"""
    assert file[:2] == b"II", file[:4]
    magic = struct.unpack_from("<H", file, 2)[0]
    big = magic == 43
    assert magic in (42, 43)
    if big:
        assert struct.unpack_from("<HH", file, 4) == (8, 0)
    os_, es, cs = (8, 20, 8) if big else (4, 12, 2)
    ifd = struct.unpack_from("<Q" if big else "<I", file, 8 if big else 4)[0]
    n = struct.unpack_from("<Q" if big else "<H", file, ifd)[0]
    tags, order = {}, []
    for q in range(n):
        ea = ifd + cs + q * es
        tag, typ, cnt = struct.unpack_from("<HHQ" if big else "<HHI", file, ea)
        size = cnt * TC.TYPE_SIZE[typ]
        pos = ea + 4 + os_ if size <= os_ else struct.unpack_from("<Q" if big else "<I", file, ea + 4 + os_)[0]
        assert pos + size <= len(file), tag
        if typ in TC.TYPE_FMT:
            tags[tag] = (typ, list(struct.unpack_from("<%d%s" % (cnt, TC.TYPE_FMT[typ]), file, pos)), pos)
            if strict and size < os_:
                assert file[pos + size:ea + 4 + 2 * os_] == bytes(os_ - size), (tag, "the value field is not zero-filled")
        order.append(tag)
    nxt = struct.unpack_from("<Q" if big else "<I", file, ifd + cs + n * es)[0]
    if strict:
        assert ifd == (16 if big else 8) and order == sorted(set(order)) and nxt == 0, (ifd, order, nxt)
    one = lambda tag, default=None: tags[tag][1][0] if tag in tags else default
    w, h, spp, bits, pred = one(256), one(257), one(277, 1), one(258), one(317, 1)
    assert tags[258][1] == [bits] * spp and one(259) == 8 and one(284, 1) == 1
    tiled = 322 in tags
    seg_w, seg_h = (one(322), one(323)) if tiled else (w, min(one(278, 0xFFFFFFFF), h))
    offs, cnts = tags[324 if tiled else 273][1], tags[325 if tiled else 279][1]
    across, down = -(-w // seg_w), -(-h // seg_h)
    assert len(offs) == len(cnts) == across * down
    segs = []
    for k, (o, cnt) in enumerate(zip(offs, cnts)):
        d = zlib.decompressobj()
        raw = d.decompress(file[o:o + cnt])
        assert d.eof and d.unused_data == b"" and o + cnt <= len(file), (k, "the segment's zlib stream")
        rows = seg_h if tiled else min(seg_h, h - (k // across) * seg_h)
        assert len(raw) == rows * seg_w * spp * (bits // 8), (k, len(raw))
        segs.append(unpredict(raw, rows, seg_w, spp, bits // 8, pred, False))
    if strict:
        assert offs[-1] + cnts[-1] == len(file), "the file does not end with the last segment"
    return tags, segs


def check_tags(tags, c, align=1):
    """the geometry tags against *w, the arrays' types, the segments at multiples of align with zero gaps judged by craft()"""
    val = lambda tag: tags[tag][1]
    seg_t = LONG8 if c.big else LONG
    assert sorted(tags) == [e[0] for e in entries(c)], sorted(tags)
    assert (val(256), val(257), val(259), val(262), val(277), val(284), val(317)) == ([c.width], [c.height], [8], [c.photometric], [c.samples], [1], [c.pred])
    assert val(258) == [c.bits] * c.samples and val(339) == [c.fmt] * c.samples
    assert all(tags[t][0] == typ for t, typ, _ in entries(c)), {t: tags[t][0] for t in tags}
    if c.extra:
        assert val(338) == [c.extra_kind] * c.extra
    if c.tile:
        assert (val(322), val(323)) == ([c.seg_w], [c.seg_h]) and tags[324][0] == tags[325][0] == seg_t
        offs = val(324)
    else:
        assert val(278) == [c.seg_h] and tags[273][0] == tags[279][0] == seg_t
        offs = val(273)
    assert len(offs) == c.n_segs and all(o % align == 0 for o in offs), offs[:8]


# ---- judge (c): PIL --------------------------------------------------------------------------------------------------------------------------
def pil_reads(c):
    """the formats PIL gives back bit for bit"""
    if c.fmt == 1 and c.bits == 8 and (c.samples, c.extra) in ((1, 0), (3, 0)):
        return True
    if c.fmt == 1 and c.bits == 8 and (c.samples, c.extra, c.extra_kind) == (4, 1, 2):
        return True
    return (c.fmt, c.bits, c.samples) in ((1, 16, 1), (3, 32, 1)) and c.extra == 0


def pil_pixels(file):
    im = Image.open(io.BytesIO(file))
    im.load()
    a = np.asarray(im)
    return a.astype(a.dtype.newbyteorder("<")).tobytes()


# ---- the target -----------------------------------------------------------------------------------------------------------------------------
class Res:
    def __init__(self, rc, file_len=None, seg_len=None, status=None, file_status=None, written=None, out=None, cap=0, clean=True):
        self.rc, self.file_len, self.seg_len, self.status, self.file_status = rc, file_len, seg_len, status, file_status
        self.written, self.out, self.cap, self.clean = written, out, cap, clean

    @property
    def file(self):
        return self.out[:self.file_len]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.tile = int(self.L.zmi_tiff_predict_tile())
        self.reader = TC.Target(L, ctx, mem)
        self.pieces = PW.Target(L, ctx, mem)                    # its payload(): the pieces through zmi_deflate_pieces_dev alone

    def bound(self, w):
        return int(self.L.zmi_tiff_bound(C.addressof(w)))

    def write(self, c, assemble=False, zero=False, pb=4096, level=6, strategy=0, align=16, shift=0, cap=None, written=True, seg_len=True,
              null=None, w=None, n_tab=None):
        """one zmi_tiff_write_dev call.  dense: the segments one behind the other with gaps of 0xEE between them, their padding noise
        (zero: zeros); cap None: zmi_tiff_bound.  w: the descriptor where it is not the case's own (the argument checks)"""
        m = self.mem
        w = w or c.desc(assemble, pb, level, strategy, align)
        n = c.n_segs if n_tab is None else n_tab
        if w.flags & ASSEMBLE:
            blob, offs = c.image, [0]
        else:
            blob, offs = bytearray(), []
            for k, s in enumerate(c.segs_zero if zero else c.segs):
                blob += b"\xEE" * (3 + k % 3)
                offs.append(len(blob))
                blob += s
        h_in = m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift)
        h_off = m.put(np.array(offs + [0], dtype=np.uint64))
        if cap is None:
            cap = self.bound(w)
        out = m.full(GUARD + cap + GUARD, FILL)
        h_fl, h_fs = m.full(16, CANARY), m.full(8, CANARY)
        h_sl, h_st, h_w = m.full((n + 1) * 4, CANARY), m.full((n + 1) * 4, CANARY), m.full(2 * 72, CANARY)
        ptr = {"ctx": self.ctx, "w": C.addressof(w), "in": h_in.ptr, "off": None if w.flags & ASSEMBLE else h_off.ptr, "out": out.ptr + GUARD,
               "fl": h_fl.ptr, "sl": h_sl.ptr if seg_len else None, "st": h_st.ptr, "fs": h_fs.ptr, "wr": h_w.ptr if written else None}
        if null:
            ptr[null] = None
        rc = self.L.zmi_tiff_write_dev(ptr["ctx"], ptr["w"], ptr["in"], ptr["off"], ptr["out"], cap, ptr["fl"], ptr["sl"], ptr["st"], ptr["fs"],
                                       ptr["wr"], m.stream)
        buf = m.read(out, np.uint8)
        fl, fs = m.read(h_fl, np.uint64), m.read(h_fs, np.int32)
        sl, st, wr = m.read(h_sl, np.uint32), m.read(h_st, np.int32), m.read(h_w, np.uint8)
        word = int.from_bytes(bytes([CANARY]) * 8, "little")
        if rc != 0:                                                          # nothing is launched: nothing is written
            untouched = bool((buf == FILL).all() and int(fl[0]) == word and (sl == word & 0xFFFFFFFF).all() and (wr == CANARY).all()
                             and (st.view(np.uint32) == word & 0xFFFFFFFF).all() and (fs.view(np.uint32) == word & 0xFFFFFFFF).all())
            return Res(rc, clean=untouched)
        clean = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all() and int(fl[1]) == word and
                     int(fs.view(np.uint32)[1]) == word & 0xFFFFFFFF and int(sl[n]) == word & 0xFFFFFFFF and
                     int(st.view(np.uint32)[n]) == word & 0xFFFFFFFF and (wr[72:] == CANARY).all() and
                     (seg_len or (sl == word & 0xFFFFFFFF).all()) and (written or (wr == CANARY).all()))
        return Res(0, int(fl[0]), [int(x) for x in sl[:n]], [int(x) for x in st[:n]], int(fs[0]), wr[:72].tobytes() if written else None,
                   buf[GUARD:GUARD + cap].tobytes(), cap, clean)

    def streams(self, c, segs, pb, level, strategy):
        """judge (b)'s segment streams"""
        out = []
        for k in range(c.n_segs):
            raw = c.predicted(segs, k)
            out.append(zlib_header(level, strategy) + self.pieces.payload(raw, pb, level, strategy) + struct.pack(">I", zlib.adler32(raw)))
        return out

    def read_back(self, file, c, segs, written):
        """judge (d)"""
        t = self.reader
        d = t.directory(types.SimpleNamespace(blob=file, pages=[None]), shift=3)
        assert d.rc == 0 and (int(d.info["status"]), int(d.info["n_pages"]), int(d.info["bigtiff"])) == (0, 1, int(c.big)), d.info
        assert int(d.rec[0]["status"]) == 0, d.rec[0]
        if written is not None:
            assert d.rec[:1].tobytes() == written, (d.rec[0], np.frombuffer(written, dtype=PAGE)[0])
        r = t.read(d, flags=0, align=16)
        assert r.rc == 0 and r.status == [0] * c.n_segs and r.detail == [0] * c.n_segs, (r.status, r.detail)
        assert all(bytes(r.slot(k)) == segs[k] for k in range(c.n_segs)), "the reader's dense regions"
        r = t.read(d, flags=ASSEMBLE)
        assert r.rc == 0 and r.status == [0] * c.n_segs, r.status
        assert bytes(r.out[:len(c.image)]) == c.image, "the reader's assembled image"


def check(t, r, c, segs, pb=4096, level=6, strategy=0, align=16, exact=None, pil=True, back=True):
    """every judge on a call that had room for its file; -> the file"""
    assert r.rc == 0 and r.clean, (r.rc, r.clean)
    assert r.file_status == 0 and r.status == [0] * c.n_segs, (r.file_status, r.status)
    assert r.file_len <= r.cap
    f = r.file
    tags, got = parse(f)                                                                      # (a)
    check_tags(tags, c, align)
    for k in range(c.n_segs):
        if got[k] != segs[k]:
            bad = next(q for q in range(len(segs[k])) if got[k][q] != segs[k][q])
            raise AssertionError("segment %d of %dx%d x%d @%d predictor %d: byte %d (row %d, column byte %d) is %d, not %d"
                                 % (k, c.width, c.height, c.samples, c.bits, c.pred, bad, bad // (c.seg_w * c.pb), bad % (c.seg_w * c.pb),
                                    got[k][bad], segs[k][bad]))
    cnts = tags[325 if c.tile else 279][1]
    assert r.seg_len == cnts, (r.seg_len[:8], cnts[:8])
    if level in EXACT if exact is None else exact:                                            # (b)
        want = craft(c, t.streams(c, segs, pb, level, strategy), align)
        assert f == want, (len(f), len(want), next((q for q in range(min(len(f), len(want))) if f[q] != want[q]), None))
    else:                                                                                     # the gaps are zero at every level
        offs = tags[324 if c.tile else 273][1]
        covered = np.zeros(len(f), dtype=bool)
        for o, n in zip(offs, cnts):
            covered[o:o + n] = True
        meta_end = min(offs)
        body = np.frombuffer(f, dtype=np.uint8)[meta_end:]
        assert not body[~covered[meta_end:]].any(), "a gap byte is not 0"
    if pil and HAVE_PIL and pil_reads(c):                                                     # (c)
        assert pil_pixels(f) == c.image, "PIL"
    if back:                                                                                  # (d)
        t.read_back(f, c, segs, r.written)
    return f


def run(t, c, assemble=False, zero=False, **kw):
    wkw = {k: v for k, v in kw.items() if k in ("pb", "level", "strategy", "align", "shift", "cap", "written", "seg_len")}
    ckw = {k: v for k, v in kw.items() if k in ("pb", "level", "strategy", "align", "exact", "pil", "back")}
    r = t.write(c, assemble=assemble, zero=zero, **wkw)
    return check(t, r, c, c.segs_zero if assemble or zero else c.segs, **ckw)


def both(t, c, **kw):
    """the page dense (noise in the padding) and assembled"""
    run(t, c, **kw)
    run(t, c, assemble=True, **kw)
    return 1


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------------
PIXELS = ((1, 8, 1, 2), (3, 8, 1, 2), (4, 8, 1, 2), (3, 16, 1, 2), (4, 16, 2, 2), (1, 64, 3, 2), (1, 32, 3, 3))


def geometry(t, tiles=((16, 16), (16, 32)), pixels=PIXELS):
    """tiles of 16 x 16 and 16 x 32 on pages of k * tile, k * tile +- 1, 1 x 1 and one tile; strips with rows_per_strip 1, 3, height, 0
    and above the height; row bytes at zmi_tiff_predict_tile() - 1, + 0, + 1 and 2 x + 1 for pixels of 1, 3, 4, 6 and 8 bytes and one
    64-bit sample under predictor 2, and for float32 under predictor 3.  Every page dense and assembled"""
    n = 0
    for tw, th in tiles:
        for k, (w, h) in enumerate(((2 * tw, 2 * th), (2 * tw - 1, 2 * th + 1), (2 * tw + 1, 2 * th - 1), (1, 1), (tw, th))):
            n += both(t, Case(w, h, 3, pred=2, tile=(tw, th), seed=10 + k, big=bool(k & 1)))
    for k, rps in enumerate((1, 3, 7, 0, 1000)):
        c = Case(9, 7, 3, pred=2, rps=rps, seed=20 + k)
        assert c.n_segs == (7, 3, 1, 1, 1)[k] and c.rows[-1] == (1, 1, 7, 7, 7)[k]
        n += both(t, c, align=1)
    T = t.tile
    for samples, bits, fmt, pred in pixels:
        pb = samples * bits // 8
        for k, rb in enumerate((T - 1, T, T + 1, 2 * T + 1)):
            w = max(1, (rb + pb - 1) // pb) if k >= 2 else max(1, rb // pb)
            n += both(t, Case(w, 3, samples, bits, fmt, pred, rps=2, seed=rb + pb), align=1)
    return n


# ---- 2. every format ------------------------------------------------------------------------------------------------------------------------
def format_cases(depths=(8, 16, 32, 64), sample_counts=(1, 2, 3, 4)):
    """every (depth, samples, predictor) the rules accept, then 5, 7 and 8 samples; the sample format follows tiff_checks.format_cases"""
    cases = [(b, s, p, f) for b, s, p, be, f in TC.format_cases(depths, sample_counts, orders=(False,))]
    return cases + [(16, 5, 2, 1), (8, 8, 2, 1), (64, 8, 2, 3), (32, 8, 3, 3), (16, 7, 3, 3), (8, 5, 1, 1), (32, 7, 2, 2)]


def formats(t, **kw):
    """pages of 21 x 7 pixels in tiles of 16 x 16, full-range samples so that every difference wraps, classic and BigTIFF in turn; the
    five formats PIL reads as strips and tiles on top"""
    n = 0
    for k, (bits, samples, pred, fmt) in enumerate(format_cases(**kw)):
        n += both(t, Case(21, 7, samples, bits, fmt, pred, tile=(16, 16), big=bool(k & 1), extra=1 if samples in (2, 4) else 0, seed=bits + samples * 3 + pred))
    for k, (samples, bits, fmt, pred, extra) in enumerate(((1, 8, 1, 2, 0), (3, 8, 1, 2, 0), (4, 8, 1, 2, 1), (1, 16, 1, 2, 0), (1, 32, 3, 3, 0))):
        c = Case(37, 21, samples, bits, fmt, pred, tile=(16, 16) if k & 1 else None, rps=None if k & 1 else 8, extra=extra, seed=50 + k)
        assert pil_reads(c)
        n += both(t, c)
    return n


# ---- 3. dense against assemble --------------------------------------------------------------------------------------------------------------
def dense_and_assemble(t, shifts=SHIFTS):
    """the same page both ways with the input at every shift: the files are equal where the dense padding is 0; with noise there the dense
    file keeps it"""
    n = 0
    for c in (Case(37, 21, 3, 16, pred=2, tile=(16, 16), seed=1), Case(21, 37, 1, 32, 3, 3, tile=(16, 32), seed=2, big=True)):
        assert c.segs != c.segs_zero
        first = None
        for shift in shifts:
            a = run(t, c, assemble=True, shift=shift, back=shift == shifts[0])
            z = run(t, c, zero=True, shift=shift, back=False)
            d = run(t, c, shift=shift, back=shift == shifts[0])
            assert a == z and d != a, shift
            first = first or (a, d)
            assert (a, d) == first, ("the file depends on the alignment of d_in", shift)
            n += 1
    return n


# ---- 4. pieces ------------------------------------------------------------------------------------------------------------------------------
def pieces(t, levels=(1, 6, 9, 0)):
    """40 x 40 RGB in tiles of 16 x 16 (768 bytes a segment): piece_bytes of 256, the segment size, that - 1 and + 1, and larger than the
    page; a strip page whose last strip is shorter"""
    n = 0
    c, s = Case(40, 40, 3, pred=2, tile=(16, 16), seed=3), Case(30, 10, 3, 16, pred=2, rps=4, seed=4)
    for level in levels:
        for pb in (256, 768, 767, 769, 1 << 20):
            run(t, c, pb=pb, level=level)
            n += 1
        run(t, s, pb=100, level=level, align=2)
        n += 1
    return n


# ---- 5. launch groups ----------------------------------------------------------------------------------------------------------------------
def launch_group(t, limit, c, pb):
    """pieces a launch group holds under a scratch limit, as png_write_checks.launch_group works it out, for the longest piece the
    page has: a full segment, or pb where that is less"""
    return PW.launch_group(t, limit, pb, min(pb, len(c.segs[0])))


def across_groups(t, c, pb, level, group, group_of, exact=None):
    """the page in one launch group, then in groups of `group` pieces (group_of(True) arranges that, group_of(False) undoes it): the
    same bytes.  That the page's pieces need at least three such groups is asserted"""
    n_pieces = sum(-(-len(s) // pb) for s in c.segs)
    assert group >= 1 and -(-n_pieces // group) >= 3, (n_pieces, group)
    one = run(t, c, pb=pb, level=level, exact=exact)
    group_of(True)
    try:
        many = run(t, c, pb=pb, level=level, exact=False, back=False)
    finally:
        group_of(False)
    assert one == many, "the file depends on the launch grouping"
    return 1


# ---- 6. determinism -------------------------------------------------------------------------------------------------------------------------
def determinism(t, levels=(6,)):
    """the same call twice and at the other alignments of d_in; the read-back runs under the decode-kernel selection the caller set"""
    n = 0
    for level in levels:
        c = Case(50, 40, 3, 8, pred=2, tile=(16, 16), seed=5 + level)
        first = run(t, c, level=level, pb=512)
        for shift in (0, 1, 3, 15):
            r = t.write(c, level=level, pb=512, shift=shift)
            assert r.rc == 0 and r.file == first, ("the file differs from the first call's", shift)
            n += 1
    return n


# ---- 7. align, inline arrays ----------------------------------------------------------------------------------------------------------------
def aligns(t, values=(1, 2, 16, 4096)):
    n = 0
    for big in (False, True):
        for a in values:
            run(t, Case(40, 33, 1, 16, pred=2, tile=(16, 16), big=big, seed=a), align=a)
            n += 1
    return n


def inline_arrays(t):
    """one-segment pages: the two arrays stand in their entries"""
    n = 0
    for big in (False, True):
        for tile in (None, (16, 16)):
            c = Case(13, 11, 3, pred=2, tile=tile, big=big, seed=7)
            assert c.n_segs == 1
            f = run(t, c, align=1)
            tags, _ = parse(f)
            os_, es, cs, ifd = (8, 20, 8, 16) if big else (4, 12, 2, 8)
            for tag in ((324, 325) if tile else (273, 279)):
                q = sorted(tags).index(tag)
                assert tags[tag][2] == ifd + cs + q * es + 4 + os_, (tag, "not inline")
            n += 1
    return n


# ---- 8. arguments ---------------------------------------------------------------------------------------------------------------------------
def arguments(t):
    """every ZMI_E_ARG of the header's list, one case each: the call returns it, zmi_tiff_bound is 0, and nothing is written"""
    c = Case(20, 20, 3, 8, pred=2, tile=(16, 16), seed=8)
    f32 = Case(20, 20, 1, 32, 3, 3, tile=(16, 16), seed=9)
    bad = [(c, dict(width=0)), (c, dict(height=0)), (c, dict(bits=12)), (c, dict(bits=0)), (c, dict(samples=0)), (c, dict(samples=9)),
           (c, dict(extra_samples=3)), (c, dict(predictor=0)), (c, dict(predictor=4)), (c, dict(predictor=3)), (f32, dict(sample_format=1)),
           (f32, dict(bits=8, sample_format=3)), (c, dict(sample_format=0)), (c, dict(sample_format=4)), (c, dict(tile_w=0)), (c, dict(tile_h=0)),
           (c, dict(tile_w=24)), (c, dict(tile_h=8)), (c, dict(tile_w=1 << 15, tile_h=1 << 15)), (c, dict(piece_bytes=0)),
           (c, dict(piece_bytes=(1 << 30) + 1)), (c, dict(level=-2)), (c, dict(level=10)), (c, dict(strategy=-1)), (c, dict(strategy=5)),
           (c, dict(out_align=0)), (c, dict(out_align=24)), (c, dict(out_align=8192)), (c, dict(flags=4)),
           (c, dict(width=1 << 16, height=1 << 16, piece_bytes=1))]
    n = 0
    for case, over in bad:
        w = case.desc(**over)
        assert t.bound(w) == 0, over
        r = t.write(case, w=w, cap=4096, n_tab=case.n_segs)
        assert r.rc == E_ARG and r.clean and t.L.zmi_last_error(), over
        n += 1
    for null in ("ctx", "w", "in", "off", "out", "fl", "st", "fs"):
        r = t.write(c, null=null, cap=4096)
        assert r.rc == E_ARG and r.clean, null
        n += 1
    assert t.L.zmi_tiff_bound(None) == 0
    return n


# ---- 9. capacity ----------------------------------------------------------------------------------------------------------------------------
def capacity(t):
    """the bound, the exact length, one byte less (Z_BUF_ERROR) and 0: *d_file_len is the need every time, nothing outside
    d_out[0 .. out_cap) is written, d_written is zeros with the status"""
    n = 0
    for c in (Case(40, 40, 3, pred=2, tile=(16, 16), seed=11), Case(30, 10, 1, 32, 3, 3, rps=4, big=True, seed=12)):
        full = t.write(c)
        f = check(t, full, c, c.segs)
        need = len(f)
        assert need <= t.bound(c.desc())
        r = t.write(c, cap=need)
        assert check(t, r, c, c.segs, back=False) == f
        n += 2
        for cap in (need - 1, 0):
            r = t.write(c, cap=cap)
            assert r.rc == 0 and r.clean and r.file_len == need and r.file_status == Z_BUF_ERROR, (cap, r.file_len, r.file_status)
            z = np.zeros(1, dtype=PAGE)
            z[0]["status"] = Z_BUF_ERROR
            assert r.written == z.tobytes() and r.status == [0] * c.n_segs and r.seg_len == full.seg_len
            n += 1
        r = t.write(c, written=False, seg_len=False)
        assert r.rc == 0 and r.clean and r.file == f
    return n
