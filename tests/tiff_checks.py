"""Checks of the TIFF reader (zmi_tiff_directory_dev / zmi_tiff_read_dev, include/zmi355.h), shared by tests/test_emu_tiff.py (CPU, the
emulator build) and tests/test_gpu_tiff.py (the MI355X), both through the C ABI on buffers a `mem` object owns (put / full / read /
stream, as in tests/zip_checks.py).

The judges are pieces of code in this file, none of them the code under test: the crafter (struct.pack, zlib, forward predictors of
its own; II / MM, classic / BigTIFF, tiles or strips, any array type, shuffled tags, placed faults) and `unpredict`, a plain numpy
reference written from TIFF 6.0 section 14 and Adobe Technical Note 3.  tests/test_tiff_craft.py pins both against PIL where PIL
imports with libtiff, and against each other everywhere.  What a faulty zlib stream must report is judged by zlib.decompressobj."""
import ctypes as C
import struct
import zlib

import numpy as np

Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR, Z_VERSION_ERROR, E_ARG = -3, -4, -5, -6, -103
TA_HEADER, TA_CHAIN = 1, 2
TP_TAGS, TP_FORMAT, TP_COMPRESSION, TP_PLANAR, TP_BIG, TE_OUT, TE_BOUNDS, TE_DATA, TE_LENGTH, TE_SPARSE = range(1, 11)
ASSEMBLE = 1
PAGES_MAX = 65535
GUARD, FILL, CANARY = 64, 0xC7, 0x77
PAGE = np.dtype([("offsets_pos", "<u8"), ("counts_pos", "<u8"), ("width", "<u4"), ("height", "<u4"), ("seg_w", "<u4"), ("seg_h", "<u4"),
                 ("segs_across", "<u4"), ("segs_down", "<u4"), ("n_segs", "<u4"), ("seg_bytes", "<u4"), ("bits", "<u2"), ("samples", "<u2"),
                 ("sample_format", "<u2"), ("predictor", "<u2"), ("compression", "<u2"), ("photometric", "<u2"), ("extra_samples", "<u2"),
                 ("sample_bytes", "u1"), ("big_endian", "u1"), ("bigtiff", "u1"), ("tiled", "u1"), ("offsets_type", "u1"),
                 ("counts_type", "u1"), ("status", "<i4")])
INFO = np.dtype([("n_pages", "<u8"), ("n_listed", "<u8"), ("first_ifd", "<u8"), ("big_endian", "<u4"), ("bigtiff", "<u4"),
                 ("status", "<i4"), ("detail", "<i4")])
assert PAGE.itemsize == 72 and INFO.itemsize == 40
SHIFTS = [0, 1, 3, 15]
BYTE, SHORT, LONG, LONG8 = 1, 3, 4, 16
TYPE_FMT = {BYTE: "B", SHORT: "H", LONG: "I", LONG8: "Q"}
TYPE_SIZE = {BYTE: 1, SHORT: 2, LONG: 4, LONG8: 8, 2: 1, 5: 8}
FLAG_STATUS = {TP_TAGS: Z_DATA_ERROR, TP_FORMAT: Z_DATA_ERROR, TP_COMPRESSION: Z_VERSION_ERROR, TP_PLANAR: Z_VERSION_ERROR,
               TP_BIG: Z_VERSION_ERROR}


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_tiff_row_tile.restype = u32
    L.zmi_tiff_row_tile.argtypes = []
    L.zmi_tiff_directory_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_tiff_read_dev.argtypes = [vp, vp, u64, vp, u32, u32, vp, u32, u64, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_ctx_set_inflate_out_limit.argtypes = [vp, u64]
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    return L


# ---- the reference unpredict and the crafter's forward predictors -----------------------------------------------------------------------
def unpredict(data, rows, seg_w, samples, sb, pred, be):
    """the decoded bytes of a segment -> its samples, little-endian, [rows, seg_w, samples] (TIFF 6.0 section 14; Technical Note 3)"""
    n = seg_w * samples
    assert len(data) == rows * n * sb
    if pred == 3:
        q = np.frombuffer(data, dtype=np.uint8).reshape(rows, seg_w * sb, samples)
        p = np.cumsum(q, axis=1, dtype=np.uint8).reshape(rows, sb, n)          # p[r, b, k]: byte b of sample k, b = 0 the most significant
        return np.ascontiguousarray(p[:, ::-1, :].transpose(0, 2, 1)).tobytes()
    d = np.frombuffer(data, dtype=(">" if be else "<") + "u%d" % sb).reshape(rows, seg_w, samples)
    if pred == 2:
        d = np.cumsum(d, axis=1, dtype=np.dtype("u%d" % sb))
    return d.astype("<u%d" % sb).tobytes()


def predict(le, rows, seg_w, samples, sb, pred, be):
    """the inverse, written on its own: the samples (little-endian bytes) -> the bytes a writer hands to the compressor"""
    n = seg_w * samples
    x = np.frombuffer(le, dtype="<u%d" % sb).reshape(rows, seg_w, samples)
    if pred == 3:
        planes = x.astype(">u%d" % sb).view(np.uint8).reshape(rows, n, sb).transpose(0, 2, 1).reshape(rows, seg_w * sb, samples)
        q = planes.copy()
        q[:, 1:, :] = planes[:, 1:, :] - planes[:, :-1, :]
        return q.tobytes()
    d = x.copy()
    if pred == 2:
        d[:, 1:, :] = x[:, 1:, :] - x[:, :-1, :]
    return d.astype((">" if be else "<") + "u%d" % sb).tobytes()


def samples_of(n, sb, seed):
    """n samples of sb bytes, full range, so that every sum of predictor 2 wraps; little-endian bytes"""
    return np.random.RandomState(seed).randint(0, 256, n * sb).astype(np.uint8).tobytes()


class Page:
    """One crafted page.  tile = (tile_w, tile_h) or None for strips of rps rows (None: the tag is left out, one strip).  arrays: the
    value type of the two arrays.  Faults and oddities: sparse (segments written with byte count 0), stream = {k: bytes} (the stored
    bytes of segment k), entry = {k: (offset or None, count or None)} (the arrays' values), tags = {tag: (type, [values]) or
    (type, [values], position) or None} (override a tag; say where its values stand without writing them; drop it), extra =
    [(tag, type, [values])].  `segs[k]` = the decoded bytes of segment k (little-endian, predictor
    undone, padding included), `image` = the page's [H, W, C] bytes; flag / expect[k] = what the reader must say."""

    def __init__(self, width, height, samples=1, bits=8, fmt=1, pred=1, comp=8, tile=None, rps=None, arrays=LONG, seed=1, level=6,
                 sparse=(), stream=None, entry=None, tags=None, extra=(), photometric=None):
        self.width, self.height, self.samples, self.bits, self.fmt, self.pred, self.comp = width, height, samples, bits, fmt, pred, comp
        self.tile, self.arrays, self.level, self.sparse = tile, arrays, level, set(sparse)
        self.stream, self.entry, self.tags, self.extra = dict(stream or {}), dict(entry or {}), dict(tags or {}), list(extra)
        self.sb = sb = bits // 8
        self.pb = samples * sb
        self.rps = rps
        self.seg_w, self.seg_h = tile if tile else (width, min(rps, height) if rps else height)
        self.across, self.down = -(-width // self.seg_w), -(-height // self.seg_h)
        self.n_segs = self.across * self.down
        self.photometric = photometric if photometric is not None else (2 if samples >= 3 else 1)
        # the padded canvas: the image in its top left corner, noise in the padding of edge tiles
        ch, cw = (self.down * self.seg_h, self.across * self.seg_w) if tile else (height, width)
        canvas = np.frombuffer(samples_of(ch * cw * samples, sb, seed), dtype=np.uint8).reshape(ch, cw, self.pb)
        self.image = np.ascontiguousarray(canvas[:height, :width]).tobytes()
        self.segs, self.rows = [], []
        for k in range(self.n_segs):
            ty, tx = divmod(k, self.across)
            rows = self.seg_h if tile else min(self.seg_h, height - ty * self.seg_h)
            seg = np.ascontiguousarray(canvas[ty * self.seg_h:ty * self.seg_h + rows, tx * self.seg_w:(tx + 1) * self.seg_w]).tobytes()
            if k in self.sparse:
                seg = bytes(len(seg))
            self.segs.append(seg)
            self.rows.append(rows)
        if self.sparse:
            img = np.frombuffer(self.image, dtype=np.uint8).reshape(height, width, self.pb).copy()
            for k in self.sparse:
                ty, tx = divmod(k, self.across)
                img[ty * self.seg_h:(ty + 1) * self.seg_h, tx * self.seg_w:(tx + 1) * self.seg_w] = 0
            self.image = img.tobytes()
        self.flag = 0
        self.expect = {k: (0, TE_SPARSE) for k in self.sparse}

    def flagged(self, code):
        self.flag = code
        return self

    def fails(self, k, detail, status=Z_DATA_ERROR):
        self.expect[k] = (status, detail)
        return self

    def stored(self, k, be):
        """the bytes of segment k as the file holds them"""
        if k in self.stream:
            return self.stream[k]
        if k in self.sparse:
            return b""
        raw = predict(self.segs[k], self.rows[k], self.seg_w, self.samples, self.sb, self.pred, be)
        assert unpredict(raw, self.rows[k], self.seg_w, self.samples, self.sb, self.pred, be) == self.segs[k]   # the crafter against the reference
        return raw if self.comp == 1 else zlib.compress(raw, self.level)

    def cropped(self, k):
        """(row, column, rows, columns) of segment k's part of the image"""
        ty, tx = divmod(k, self.across)
        return (ty * self.seg_h, tx * self.seg_w, min(self.seg_h, self.height - ty * self.seg_h), min(self.seg_w, self.width - tx * self.seg_w))


class Tiff:
    """One crafted file of several pages: header | per page: the segments, the out-of-line values, the IFD.  shuffle: the tags of every
    IFD in an order that is not ascending; odd: every segment at an odd offset; chain = {i: offset}: the next-IFD word of IFD i."""

    def __init__(self, pages, be=False, big=False, shuffle=False, odd=False, chain=None, header=None, n_entries=None):
        self.pages, self.be, self.big = pages, be, big
        e = self.e = ">" if be else "<"
        os_ = 8 if big else 4
        out = bytearray((b"MM" if be else b"II") + (struct.pack(e + "HHHQ", 43, 8, 0, 0) if big else struct.pack(e + "HI", 42, 0)))
        first_at = 8 if big else 4
        link_at = first_at                                                 # where the offset of the next IFD is to be written
        self.ifd_pos, self.records, links = [], [], []
        for i, p in enumerate(pages):
            offs, cnts = [], []
            for k in range(p.n_segs):
                data = p.stored(k, be)
                if odd and len(out) % 2 == 0:
                    out += b"\xA5"
                offs.append(len(out) if data else 0)
                cnts.append(len(data))
                out += data
            for k, (o, c) in p.entry.items():
                offs[k] = offs[k] if o is None else o
                cnts[k] = cnts[k] if c is None else c
            ent = {256: (LONG, [p.width]), 257: (LONG, [p.height]), 258: (SHORT, [p.bits] * p.samples), 259: (SHORT, [p.comp]),
                   262: (SHORT, [p.photometric]), 277: (SHORT, [p.samples]), 284: (SHORT, [1]), 339: (SHORT, [p.fmt] * p.samples)}
            if p.pred != 1:
                ent[317] = (SHORT, [p.pred])
            if p.samples in (2, 4):
                ent[338] = (SHORT, [2])
            if p.tile:
                ent.update({322: (SHORT, [p.seg_w]), 323: (LONG, [p.seg_h]), 324: (p.arrays, offs), 325: (p.arrays, cnts)})
            else:
                ent.update({273: (p.arrays, offs), 279: (p.arrays, cnts)})
                if p.rps:
                    ent[278] = (LONG, [p.rps])
            ent[305] = (2, list(b"crafted\0"))                                # an ASCII tag the reader skips
            for tag, v in p.tags.items():
                if v is None:
                    ent.pop(tag, None)
                else:
                    ent[tag] = v
            for tag, typ, vals in p.extra:
                ent[tag] = (typ, vals)
            order = sorted(ent)
            if shuffle:
                order = order[1::2] + order[0::2][::-1]
            fields, rec_pos = [], {}
            for tag in order:
                typ, vals = ent[tag][:2]
                if len(ent[tag]) == 3:                                    # (type, values, position): the values are said to stand there
                    fields.append((tag, typ, len(vals), struct.pack(e + ("Q" if big else "I"), ent[tag][2]), False))
                    continue
                raw = bytes(vals) if typ == 2 else struct.pack(e + "%d%s" % (len(vals), TYPE_FMT[typ]), *vals)
                if len(raw) <= os_:
                    fields.append((tag, typ, len(vals), raw.ljust(os_, b"\0"), True))
                else:
                    if len(out) % 2:
                        out += b"\0"
                    rec_pos[tag] = len(out)
                    fields.append((tag, typ, len(vals), struct.pack(e + ("Q" if big else "I"), len(out)), False))
                    out += raw
            if len(out) % 2:
                out += b"\0"
            at = len(out)
            self.ifd_pos.append(at)
            struct.pack_into(e + ("Q" if big else "I"), out, link_at, at)
            ne = len(fields) if n_entries is None else n_entries
            out += struct.pack(e + ("Q" if big else "H"), ne)
            for q, (tag, typ, cnt, field, inline) in enumerate(fields):
                ea = len(out)
                out += struct.pack(e + ("HHQ" if big else "HHI"), tag, typ, cnt) + field
                if inline:
                    rec_pos[tag] = ea + 4 + os_
            link_at = len(out)
            out += struct.pack(e + ("Q" if big else "I"), 0)
            ot, ct = (324, 325) if p.tile else (273, 279)
            self.records.append(dict(offsets_pos=rec_pos.get(ot, 0), counts_pos=rec_pos.get(ct, 0), offs=offs, cnts=cnts))
            links.append(link_at)
        for i, to in (chain or {}).items():
            struct.pack_into(e + ("Q" if big else "I"), out, links[i], to)
        if header:
            out[:len(header)] = header
        self.blob = bytes(out)
        self.info = (0, 0)                                                 # status, detail of the directory
        self.n_pages = len(pages)

    def broken(self, detail, n_pages):
        self.info, self.n_pages = (Z_DATA_ERROR, detail), n_pages
        return self


def judge_stream(payload, n):
    """what zlib says of a stream that must give exactly n bytes"""
    d = zlib.decompressobj()
    try:
        raw = d.decompress(payload, n + 1)
    except zlib.error:
        return Z_DATA_ERROR, TE_DATA
    if len(raw) != n or not d.eof:
        return Z_DATA_ERROR, TE_LENGTH
    return 0, 0


# ---- the target ---------------------------------------------------------------------------------------------------------------------------
class Dir:
    def __init__(self, rc, info, rec, h_in, h_pages, tiff, cap):
        self.rc, self.info, self.rec, self.h_in, self.h_pages, self.tiff, self.cap = rc, info, rec, h_in, h_pages, tiff, cap


class Read:
    def __init__(self, rc, off, length, status, detail, out):
        self.rc, self.off, self.len, self.status, self.detail, self.out = rc, off, length, status, detail, out

    def slot(self, j):
        return self.out[self.off[j]:self.off[j] + self.len[j]]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.row_tile = int(self.L.zmi_tiff_row_tile())

    def directory(self, tiff, shift=0, cap=None, ctx="ctx"):
        """one zmi_tiff_directory_dev call; a record of canary stands behind the table"""
        m = self.mem
        cap = len(tiff.pages) if cap is None else cap
        h_in = m.put(np.frombuffer(tiff.blob + b"\0" * 16, dtype=np.uint8), shift)
        h_pages = m.full((cap + 1) * 72, CANARY)
        h_info = m.full(40 + 8, CANARY)
        rc = self.L.zmi_tiff_directory_dev(self.ctx if ctx == "ctx" else ctx, h_in.ptr, len(tiff.blob), h_pages.ptr, cap, h_info.ptr, m.stream)
        if rc != 0:
            return Dir(rc, None, None, h_in, h_pages, tiff, cap)
        raw = m.read(h_info, np.uint8)
        assert bytes(raw[40:]) == bytes([CANARY]) * 8, "the call wrote behind its info"
        rec = m.read(h_pages, PAGE)
        assert bytes(rec[cap:].tobytes()) == bytes([CANARY]) * 72, "the call wrote behind its table"
        return Dir(rc, raw[:40].view(INFO)[0], rec[:cap], h_in, h_pages, tiff, cap)

    def read(self, d, page=0, sel=None, n_sel=None, flags=0, align=1, cap=None, decoded=None, n_pages=None, null=None, ctx="ctx", pages=None):
        """one zmi_tiff_read_dev call; cap None: exactly the room the selection needs, decoded None: exactly the sum"""
        m = self.mem
        n_pages = d.cap if n_pages is None else n_pages
        rec = d.rec if pages is None else pages
        p = rec[page] if page < n_pages else None
        if n_sel is None:
            n_sel = (int(p["n_segs"]) if p is not None and int(p["status"]) == 0 else 1) if sel is None else len(sel)
        plan_off, plan_size = plan(p, sel, n_sel, align, flags)
        need = plan_off[-1]
        cap = need if cap is None else cap
        decoded = sum(dense_size(p, j if sel is None else sel[j]) for j in range(n_sel)) if decoded is None else decoded
        h_sel = m.put(np.array(list(sel) + [0], dtype=np.uint32)) if sel is not None else None
        h_out = m.full(GUARD + cap + GUARD, FILL)
        h_o = m.full((n_sel + 2) * 8, CANARY)
        h_l = m.full((n_sel + 1) * 4, CANARY)
        h_s = m.full((n_sel + 1) * 4, CANARY)
        h_d = m.full((n_sel + 1) * 4, CANARY)
        args = dict(off=h_o.ptr, len=h_l.ptr, st=h_s.ptr, det=h_d.ptr)
        if null:
            args[null] = None
        h_pages = d.h_pages if pages is None else m.put(pages)
        rc = self.L.zmi_tiff_read_dev(self.ctx if ctx == "ctx" else ctx, d.h_in.ptr, len(d.tiff.blob), h_pages.ptr, n_pages, page,
                                      h_sel.ptr if h_sel else None, n_sel, decoded, flags, align, h_out.ptr + GUARD, cap, args["off"], args["len"],
                                      args["st"], args["det"], m.stream)
        if rc != 0:
            return Read(rc, None, None, None, None, None)
        off = [int(x) for x in m.read(h_o, np.uint64)]
        ln = [int(x) for x in m.read(h_l, np.uint32)]
        st = [int(x) for x in m.read(h_s, np.int32)]
        det = [int(x) for x in m.read(h_d, np.int32)]
        buf = m.read(h_out, np.uint8)
        word = int.from_bytes(bytes([CANARY]) * 8, "little")
        assert off[n_sel + 1] == word and ln[n_sel] == word & 0xFFFFFFFF and st[n_sel] == np.int32(word & 0xFFFFFFFF), "the call wrote behind its tables"
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all(), "the call wrote outside d_out[0 .. out_cap)"
        r = Read(rc, off[:n_sel + 1], ln[:n_sel], st[:n_sel], det[:n_sel], buf[GUARD:GUARD + cap])
        r.plan_off, r.plan_size, r.need, r.cap = plan_off, plan_size, need, cap
        return r


def dense_size(p, k):
    """decoded bytes of segment k of record p; 0 for what reads nothing"""
    if p is None or int(p["status"]) != 0 or k >= int(p["n_segs"]):
        return 0
    pb = int(p["samples"]) * int(p["sample_bytes"])
    rows = int(p["seg_h"])
    if not int(p["tiled"]):
        rows = min(rows, int(p["height"]) - (k // int(p["segs_across"])) * rows)
    return rows * int(p["seg_w"]) * pb


def plan(p, sel, n_sel, align, flags):
    """the offsets the contract gives.  dense: the decoded sizes of the slots in front that read a segment, each rounded up to align, then
    the need; assemble: the offset of every segment's first pixel, then the image's size"""
    off, sizes, at = [], [], 0
    align = align if 1 <= align <= 4096 and not align & (align - 1) else 1
    ok = p is not None and int(p["status"]) == 0
    for j in range(n_sel):
        k = j if sel is None else sel[j]
        size = dense_size(p, k)
        if flags & ASSEMBLE:
            pb = int(p["samples"]) * int(p["sample_bytes"]) if ok else 0
            ty, tx = divmod(k, int(p["segs_across"])) if size else (0, 0)
            off.append((ty * int(p["seg_h"]) * int(p["width"]) + tx * int(p["seg_w"])) * pb if size else 0)
        else:
            off.append(at)
        sizes.append(size)
        at += -(-size // align) * align
    if flags & ASSEMBLE:
        at = int(p["width"]) * int(p["height"]) * int(p["samples"]) * int(p["sample_bytes"]) if ok else 0
    return off + [at], sizes


# ---- judges ---------------------------------------------------------------------------------------------------------------------------------
def check_directory(d, n_listed=None):
    """the info and every listed record against what the crafter wrote"""
    t = d.tiff
    assert d.rc == 0
    assert (int(d.info["status"]), int(d.info["detail"])) == t.info, (int(d.info["status"]), int(d.info["detail"]), t.info)
    if t.info[1] & 0xFF == TA_HEADER:
        assert int(d.info["n_pages"]) == 0 and int(d.info["n_listed"]) == 0
        return
    assert int(d.info["n_pages"]) == t.n_pages and int(d.info["n_listed"]) == min(t.n_pages, d.cap), (int(d.info["n_pages"]), t.n_pages)
    assert (int(d.info["big_endian"]), int(d.info["bigtiff"])) == (int(t.be), int(t.big))
    assert t.info != (0, 0) or int(d.info["first_ifd"]) == t.ifd_pos[0]
    for i in range(min(t.n_pages, d.cap, len(t.pages))):
        e, p, w = d.rec[i], t.pages[i], t.records[i]
        assert int(e["status"]) == p.flag, (i, int(e["status"]), p.flag)
        assert (int(e["big_endian"]), int(e["bigtiff"])) == (int(t.be), int(t.big))
        if p.flag == TP_TAGS:
            continue
        got = tuple(int(e[f]) for f in ("width", "height", "photometric", "tiled"))       # a flagged page is listed with its dimensions
        assert got == (p.width, p.height, p.photometric, int(bool(p.tile))), (i, got)
        if p.flag == 0:
            assert (int(e["samples"]), int(e["compression"])) == (p.samples, p.comp)
            got = tuple(int(e[f]) for f in ("seg_w", "seg_h", "segs_across", "segs_down", "n_segs", "seg_bytes", "bits", "sample_format",
                                            "predictor", "sample_bytes", "offsets_pos", "counts_pos", "offsets_type", "counts_type", "extra_samples"))
            assert got == (p.seg_w, p.seg_h, p.across, p.down, p.n_segs, p.seg_w * p.seg_h * p.pb, p.bits, p.fmt, p.pred, p.sb,
                           w["offsets_pos"], w["counts_pos"], p.arrays, p.arrays, 1 if p.samples in (2, 4) else 0), (i, got)
    for i in range(min(t.n_pages, d.cap), d.cap):
        assert bytes(d.rec[i:i + 1].tobytes()) == bytes([CANARY]) * 72, "a record behind n_listed was written"


def check_read(r, p, sel=None, flags=0, over=False):
    """every slot's words and bytes, the offsets, the need, and nothing written elsewhere.  p: the crafted page"""
    assert r.rc == 0
    assert r.off == r.plan_off, (r.off[:8], r.plan_off[:8])
    want = np.full(r.cap, FILL, dtype=np.uint8)
    known = np.ones(r.cap, dtype=bool)
    img_fits = r.plan_off[-1] <= r.cap
    for j in range(len(r.status)):
        k = j if sel is None else sel[j]
        size = r.plan_size[j]
        if over:
            st, det = E_ARG, 0
        elif p.flag:
            st, det = FLAG_STATUS[p.flag], p.flag
        elif k >= p.n_segs:
            st, det = E_ARG, 0
        elif not (img_fits if flags & ASSEMBLE else r.plan_off[j] + size <= r.cap):
            st, det = Z_BUF_ERROR, TE_OUT
        else:
            st, det = p.expect.get(k, (0, 0))
        assert (r.status[j], r.detail[j]) == (st, det), (j, k, r.status[j], r.detail[j], st, det)
        if size == 0 or over or (st != 0 and det == TE_OUT):
            assert r.len[j] == 0, (j, k)
            continue
        if flags & ASSEMBLE:
            r0, c0, nr, nc = p.cropped(k)
            idx = ((r0 + np.arange(nr))[:, None] * p.width + c0 + np.arange(nc)[None, :])[:, :, None] * p.pb + np.arange(p.pb)[None, None, :]
            idx = idx.reshape(-1)
            seg = np.frombuffer(p.segs[k], dtype=np.uint8).reshape(p.rows[k], p.seg_w, p.pb)[:nr, :nc].reshape(-1)
        else:
            idx = r.plan_off[j] + np.arange(size)
            seg = np.frombuffer(p.segs[k], dtype=np.uint8)
        if st == 0:
            assert r.len[j] == len(idx), (j, k, r.len[j], len(idx))
            want[idx] = seg
        else:
            assert r.len[j] == 0, (j, k)
            known[idx] = False                                             # a failed segment's region: unspecified
    got = r.out
    bad = np.nonzero((got != want) & known)[0]
    if len(bad):
        raise AssertionError("byte %d of the output is %d, not %d (%d bytes differ)" % (bad[0], got[bad[0]], want[bad[0]], len(bad)))


def run(t, tiff, shift=0, align=1, flags=None, sel=None, pages=None):
    """directory and read of every page (or `pages`) of a file, dense and assembled, everything checked"""
    d = t.directory(tiff, shift=shift)
    check_directory(d)
    for i in (range(len(tiff.pages)) if pages is None else pages):
        for fl in ((0, ASSEMBLE) if flags is None else flags):
            r = t.read(d, page=i, sel=sel, flags=fl, align=align)
            try:
                check_read(r, tiff.pages[i], sel=sel, flags=fl)
            except AssertionError as e:
                raise AssertionError("page %d flags %d: %s" % (i, fl, e))
    return d


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------------
def geometry(t, tiles=((16, 16), (16, 32)), pixels=((1, 8), (3, 8), (4, 8), (3, 16), (1, 64))):
    """tiles of 16 x 16 and 16 x 32 with images of k * tile, k * tile +- 1 and 1 x 1; strips of 1 and 5 rows, one strip (no RowsPerStrip,
    and RowsPerStrip above the height), a short last strip; row bytes around zmi_tiff_row_tile() for pixels of 1, 3, 4, 6 and 8 bytes
    under predictor 2; widths 1 and 2"""
    n = 0
    for tw, th in tiles:
        pages = []
        for k, (w, h) in enumerate(((2 * tw, 2 * th), (2 * tw - 1, 2 * th + 1), (2 * tw + 1, 2 * th - 1), (1, 1), (tw, th))):
            pages.append(Page(w, h, samples=3, pred=2, tile=(tw, th), seed=10 + k))
        run(t, Tiff(pages), align=16)
        n += len(pages)
    pages = [Page(9, 7, 3, pred=2, rps=1, seed=1), Page(9, 13, 1, 16, pred=2, rps=5, seed=2), Page(9, 7, 3, pred=2, seed=3),
             Page(9, 7, 3, pred=2, rps=1000, seed=4), Page(11, 10, 4, pred=2, rps=5, seed=5), Page(1, 9, 3, pred=2, rps=4, seed=6),
             Page(2, 3, 1, pred=2, rps=2, seed=7), Page(1, 1, 1, seed=8), Page(2, 2, 2, 16, pred=2, tile=(16, 16), seed=9)]
    assert pages[1].rows[-1] == 3 and pages[3].seg_h == 7
    run(t, Tiff(pages), align=1)
    n += len(pages)
    T = t.row_tile
    for samples, bits in pixels:
        pb = samples * bits // 8
        pages = []
        for k, rb in enumerate((T - 1, T, T + 1, 2 * T + 1)):
            w = max(1, (rb + pb - 1) // pb) if k >= 2 else max(1, rb // pb)
            pages.append(Page(w, 3, samples, bits, pred=2, rps=2, seed=rb + pb))
        run(t, Tiff(pages), align=1)
        n += len(pages)
    return n


# ---- 2. every format ------------------------------------------------------------------------------------------------------------------------
def format_cases(depths=(8, 16, 32, 64), sample_counts=(1, 2, 3, 4), orders=(False, True)):
    """every (depth, samples, predictor, byte order) the page rules accept; the sample format follows the predictor: unsigned and signed
    integers and floats under predictors 1 and 2, floats under 3"""
    cases = []
    for bits in depths:
        for samples in sample_counts:
            for pred in (1, 2, 3):
                if pred == 3 and bits < 16:
                    continue
                for be in orders:
                    fmt = 3 if pred == 3 else (1, 2, 3)[(bits // 8 + samples + pred) % 3] if bits >= 16 else (1, 2)[samples % 2]
                    cases.append((bits, samples, pred, be, fmt))
    return cases


def formats(t, **kw):
    """pages of 21 x 7 pixels in tiles of 16 x 16, full-range samples so that every sum wraps; 5 and 8 samples too"""
    cases = format_cases(**kw)
    cases += [(16, 5, 2, False, 1), (8, 8, 2, True, 1), (64, 8, 2, False, 3), (32, 8, 3, True, 3), (16, 7, 3, False, 3)]
    n = 0
    for be in sorted({c[3] for c in cases}):
        pages = [Page(21, 7, samples, bits, fmt, pred, tile=(16, 16), seed=bits + samples * 3 + pred) for bits, samples, pred, b, fmt in cases if b == be]
        run(t, Tiff(pages, be=be), align=16)
        n += len(pages)
    return n


# ---- 3. layout ------------------------------------------------------------------------------------------------------------------------------
def layout(t):
    """classic / BigTIFF x II / MM x the array types; one-element arrays (inline); shuffled tags; three pages of different formats; odd
    segment offsets; sparse segments; compression 1 and 32946; levels 0, 1 and 9"""
    n = 0
    for big in (False, True):
        for be in (False, True):
            for arrays in (SHORT, LONG, LONG8):
                pages = [Page(20, 20, 3, 8, pred=2, tile=(16, 16), arrays=arrays, seed=1), Page(7, 5, 1, 16, pred=2, arrays=arrays, seed=2)]
                run(t, Tiff(pages, be=be, big=big), align=16)
                n += 1
    three = [Page(20, 9, 3, 8, pred=2, tile=(16, 16), seed=3), Page(13, 11, 1, 32, 3, 3, rps=4, seed=4, comp=32946),
             Page(5, 6, 2, 16, 2, 1, rps=2, comp=1, seed=5)]
    for kw in (dict(shuffle=True), dict(shuffle=True, big=True, be=True), dict(odd=True), dict(odd=True, be=True, shuffle=True)):
        run(t, Tiff(three, **kw), align=1)
        n += 1
    sparse = [Page(40, 40, 3, 8, pred=2, tile=(16, 16), sparse=(0, 4, 8), seed=6), Page(9, 9, 1, 16, pred=2, rps=3, sparse=(1,), seed=7)]
    run(t, Tiff(sparse), align=16)
    n += 1
    levels = [Page(30, 30, 3, 8, pred=2, tile=(16, 16), level=lv, seed=8 + lv) for lv in (0, 1, 9)]
    run(t, Tiff(levels), align=16)
    n += 1
    return n


# ---- 4. selection and room ------------------------------------------------------------------------------------------------------------------
def selection(t):
    p = Page(50, 40, 3, 8, pred=2, tile=(16, 16), seed=11)                 # 4 x 3 tiles
    tiff = Tiff([p, Page(9, 20, 1, 16, pred=2, rps=3, seed=12)])
    n = 0
    for shift in SHIFTS:
        d = t.directory(tiff, shift=shift)
        check_directory(d)
        for sel in ([1, 3, 5], list(range(11, -1, -1)), [2, 2, 0, 2], [0, 12, 1, 4000000000, 2]):
            for fl, align in ((0, 1), (0, 16), (0, 4096), (ASSEMBLE, 1)):
                check_read(t.read(d, 0, sel=sel, flags=fl, align=align), p, sel=sel, flags=fl)
                n += 1
    d = t.directory(tiff)
    r = t.read(d, 0, sel=[], flags=0)
    assert r.rc == 0 and r.off == [0]
    check_read(t.read(d, 1, sel=[6, 0, 6], flags=0), tiff.pages[1], sel=[6, 0, 6])
    check_read(t.read(d, 1, sel=[6, 0], flags=ASSEMBLE), tiff.pages[1], sel=[6, 0], flags=ASSEMBLE)
    n += 3
    full = t.read(d, 0, align=16)
    check_read(full, p)
    for cap in (full.need - 1, full.off[2], 0):                          # one byte short; the cap cuts behind the second tile; no room
        r = t.read(d, 0, align=16, cap=cap)
        check_read(r, p)
        assert r.off[-1] == full.need and r.status.count(Z_BUF_ERROR) == sum(o + 768 > cap for o in full.off[:-1]) > 0
        n += 1
    size = 50 * 40 * 3
    for cap in (size - 1, 0):
        r = t.read(d, 0, flags=ASSEMBLE, cap=cap)
        check_read(r, p, flags=ASSEMBLE)
        assert r.off[-1] == size and r.status == [Z_BUF_ERROR] * 12 and (r.out == FILL).all()
        n += 1
    for fl in (0, ASSEMBLE):                                              # decoded_bytes one byte short: every slot, nothing written
        r = t.read(d, 0, flags=fl, decoded=12 * 768 - 1)
        check_read(r, p, flags=fl, over=True)
        assert (r.out == FILL).all()
        check_read(t.read(d, 0, flags=fl, decoded=12 * 768 + 1000), p, flags=fl)
        n += 1
    return n


# ---- 5. every status code, among good neighbours ----------------------------------------------------------------------------------------------
def header_cases():
    """-> [(name, Tiff)] for every ZMI_TA_* case"""
    def page():
        return Page(9, 7, 3, 8, pred=2, rps=3, seed=41)

    cases = []
    for name, hdr in (("byte order", b"IM"), ("magic 44", b"II" + struct.pack("<H", 44)), ("no file", None)):
        f = Tiff([page()], header=hdr).broken(TA_HEADER, 0)
        if hdr is None:
            f.blob = f.blob[:7]
        cases.append((name, f))
    f = Tiff([page()], big=True, header=b"II" + struct.pack("<HH", 43, 4)).broken(TA_HEADER, 0)
    cases.append(("bigtiff offset size 4", f))
    f = Tiff([page()], big=True, be=True, header=b"MM" + struct.pack(">HHH", 43, 8, 1)).broken(TA_HEADER, 0)
    cases.append(("bigtiff reserved word", f))
    cases.append(("second IFD leaves the file", Tiff([page(), page()], chain={0: 1 << 30}).broken(TA_CHAIN | 1 << 8, 1)))
    f = Tiff([page(), page()])
    cases.append(("second IFD cut", f.broken(TA_CHAIN | 1 << 8, 1)))
    f.blob = f.blob[:-3]
    cases.append(("IFD of 0 entries", Tiff([page()], n_entries=0).broken(TA_CHAIN | 0 << 8, 0)))
    f = Tiff([page()], header=b"II" + struct.pack("<HI", 42, 0)).broken(TA_CHAIN | 0 << 8, 0)
    cases.append(("first IFD at 0", f))
    f = Tiff([page(), page(), page()], big=True, be=True)
    g = Tiff([page(), page(), page()], big=True, be=True, chain={2: f.ifd_pos[1]}).broken(TA_CHAIN | PAGES_MAX << 8, PAGES_MAX)
    cases.append(("chain loops back", g))
    return cases


def page_cases():
    """-> [(name, Page)] for every ZMI_TP_* case: flagged pages"""
    def base(**kw):
        args = dict(samples=3, bits=8, pred=2, tile=(16, 16), seed=42)
        args.update(kw)
        return Page(20, 20, **args)

    cases = [("no width", base(tags={256: None}).flagged(TP_TAGS)), ("no height", base(tags={257: None}).flagged(TP_TAGS)),
             ("no tile offsets", base(tags={324: None}).flagged(TP_TAGS)), ("no tile length", base(tags={323: None}).flagged(TP_TAGS)),
             ("no strip counts", base(tile=None, tags={279: None}).flagged(TP_TAGS)),
             ("strips and tiles", base(extra=[(273, LONG, [8]), (279, LONG, [8])]).flagged(TP_TAGS)),
             ("neither", base(tags={322: None, 323: None, 324: None, 325: None}).flagged(TP_TAGS)),
             ("three counts for four tiles", base(tags={325: (LONG, [10, 10, 10])}).flagged(TP_TAGS)),
             ("offsets leave the file", base(tags={324: (LONG, [8] * 4, 1 << 30)}).flagged(TP_TAGS)),
             ("offsets of type BYTE", base(tags={324: (BYTE, [8] * 4)}).flagged(TP_TAGS)),
             ("zero width", base(tags={256: (LONG, [0])}).flagged(TP_TAGS)), ("zero tile width", base(tags={322: (SHORT, [0])}).flagged(TP_TAGS)),
             ("zero rows per strip", base(tile=None, rps=4, tags={278: (LONG, [0])}).flagged(TP_TAGS)),
             ("depths differ", base(tags={258: (SHORT, [8, 8, 16])}).flagged(TP_FORMAT)), ("depth 12", base(tags={258: (SHORT, [12] * 3)}).flagged(TP_FORMAT)),
             ("depth 1 by default", base(tags={258: None}).flagged(TP_FORMAT)),
             ("predictor 3 on integers", base(bits=32, tags={317: (SHORT, [3])}).flagged(TP_FORMAT)),
             ("predictor 3 at depth 8", base(fmt=3, tags={317: (SHORT, [3])}).flagged(TP_FORMAT)),
             ("predictor 4", base(tags={317: (SHORT, [4])}).flagged(TP_FORMAT)), ("nine samples", base(tags={277: (SHORT, [9])}).flagged(TP_FORMAT)),
             ("lzw", base(tags={259: (SHORT, [5])}).flagged(TP_COMPRESSION)), ("zstd", base(tags={259: (SHORT, [50000])}).flagged(TP_COMPRESSION)),
             ("planar 2", base(tags={284: (SHORT, [2])}).flagged(TP_PLANAR)),
             ("tile of 4 GiB", Page(1, 1, 1, 8, tile=(16, 16), seed=1, tags={322: (LONG, [65536]), 323: (LONG, [65536])}).flagged(TP_BIG))]
    return cases


def segment_cases():
    """-> a page of 4 x 4 tiles with a fault in every other one, and a raw page; the good tiles are the neighbours"""
    good = Page(64, 64, 3, 8, pred=2, tile=(16, 16), seed=43)
    raw = predict(good.segs[1], 16, 16, 3, 1, 2, False)
    ok = zlib.compress(raw, 6)
    n = len(raw)
    adler = ok[:-4] + struct.pack(">I", zlib.adler32(raw) ^ 1)
    corrupt = bytearray(ok)
    corrupt[len(ok) // 2] ^= 0x10
    d = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, b"a preset dictionary")
    fdict = d.compress(raw) + d.flush()
    assert fdict[1] & 0x20 and judge_stream(adler, n) == (Z_DATA_ERROR, TE_DATA)
    stream = {1: adler, 3: bytes(corrupt), 5: fdict, 7: zlib.compress(raw[:-48]), 9: zlib.compress(raw + bytes(48)), 11: ok[:len(ok) // 2], 13: ok[:1],
              15: zlib.compress(predict(good.segs[15], 16, 16, 3, 1, 2, False), 6) + b"junk behind the stream"}     # accepted
    p = Page(64, 64, 3, 8, pred=2, tile=(16, 16), seed=43, stream=stream, sparse=(6,), entry={2: (1 << 31, None), 8: (None, 1 << 30)})
    for k in (1, 3, 5, 7, 9, 11, 13):
        p.fails(k, judge_stream(stream[k], n)[1] if k != 5 else TE_DATA)
    assert [p.expect[k][1] for k in (7, 9, 11, 13)] == [TE_LENGTH] * 4 and p.expect[1][1] == TE_DATA
    p.fails(2, TE_BOUNDS).fails(8, TE_BOUNDS)
    big = Page(64, 64, 3, 8, pred=2, tile=(16, 16), seed=44, arrays=LONG8, entry={4: (None, 1 << 32), 10: ((1 << 63) + 5, None)})
    big.fails(4, TE_BOUNDS).fails(10, TE_BOUNDS)
    rawp = Page(20, 12, 2, 16, pred=2, comp=1, rps=3, seed=45, entry={1: (None, 20 * 3 * 4 - 1), 2: (None, 20 * 3 * 4 + 1)})
    rawp.fails(1, TE_LENGTH).fails(2, TE_LENGTH)
    return [p, big, rawp]


def statuses(t):
    """every ZMI_TA_* file; every ZMI_TP_* page between two good pages; every ZMI_TE_* segment between good tiles"""
    n = 0
    for name, f in header_cases():
        try:
            d = t.directory(f, cap=4)
            check_directory(d)
            for i in range(min(f.n_pages, len(f.pages))):
                check_read(t.read(d, i), f.pages[i])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        n += 1
    left, right = Page(20, 9, 3, 8, pred=2, tile=(16, 16), seed=31), Page(13, 11, 1, 32, 3, 3, rps=4, seed=32)
    cases = page_cases()
    seen = set()
    for at in range(0, len(cases), 6):
        group = cases[at:at + 6]
        f = Tiff([left] + [p for _, p in group] + [right], big=at % 12 == 6, be=at % 12 == 0)
        try:
            run(t, f, align=16)
        except AssertionError as e:
            raise AssertionError("%s: %s" % ([name for name, _ in group], e))
        seen |= {p.flag for _, p in group}
        n += len(group)
    assert seen == {TP_TAGS, TP_FORMAT, TP_COMPRESSION, TP_PLANAR, TP_BIG}
    pages = segment_cases()
    run(t, Tiff(pages), align=16)
    run(t, Tiff(pages, be=True, big=True), align=1, shift=3)
    seen = {det for p in pages for _, det in p.expect.values()}
    assert seen == {TE_BOUNDS, TE_DATA, TE_LENGTH, TE_SPARSE}, seen
    n += 2 * len(pages)
    return n


def forged_record(t):
    """a record no directory call would write for its file is ZMI_E_ARG in every slot and nothing of it is read; the page behind it reads"""
    pages = [Page(20, 20, 3, 8, pred=2, tile=(16, 16), seed=51), Page(9, 9, 1, 16, pred=2, rps=4, seed=52)]
    tiff = Tiff(pages)
    d = t.directory(tiff)
    check_directory(d)
    n = 0
    for field, value in (("offsets_pos", len(tiff.blob) - 15), ("counts_pos", 1 << 40), ("n_segs", 5), ("seg_bytes", 16 * 16 * 3 + 1), ("seg_w", 0),
                         ("sample_bytes", 3), ("samples", 9), ("counts_type", 1), ("segs_across", 3), ("compression", 5), ("predictor", 3),
                         ("status", 99), ("status", -3)):
        rec = d.rec.copy()
        rec[0][field] = value
        for fl in (0, ASSEMBLE):
            r = t.read(d, 0, n_sel=4, flags=fl, cap=4 * 768, decoded=4 * 768, pages=rec)
            assert r.rc == 0 and r.status == [E_ARG] * 4 and r.detail == [0] * 4 and r.len == [0] * 4 and (r.out == FILL).all(), (field, r.status)
            assert r.off[-1] == 0
        check_read(t.read(d, 1, pages=rec), pages[1])
        n += 1
    r = t.read(d, 2, n_sel=2, cap=64, decoded=64)                            # a page index behind the table
    assert r.rc == 0 and r.status == [E_ARG] * 2 and (r.out == FILL).all()
    return n + 1


# ---- 6. determinism, 7. arguments -------------------------------------------------------------------------------------------------------------
def determinism(t):
    """the same words and bytes whatever the alignment of d_in, the selection a segment stands in and the context's scratch limits (the
    call sizes the decoder's bitmap itself: the context's inflate limit at its smallest, 1 MiB, and its scratch limit at its smallest,
    64 MiB, change nothing)"""
    p = Page(70, 50, 3, 16, pred=2, tile=(16, 16), seed=61)
    tiff = Tiff([p, Page(33, 20, 2, 32, 3, 3, rps=3, seed=62)], be=True)
    d0 = t.directory(tiff)
    refs = {}
    for page in (0, 1):
        for fl in (0, ASSEMBLE):
            refs[page, fl] = t.read(d0, page, flags=fl, align=16)
            check_read(refs[page, fl], tiff.pages[page], flags=fl)
    n = 0

    def same(d):
        for (page, fl), ref in refs.items():
            r = t.read(d, page, flags=fl, align=16)
            assert (r.off, r.len, r.status, r.detail) == (ref.off, ref.len, ref.status, ref.detail) and (r.out == ref.out).all()

    assert t.L.zmi_ctx_set_inflate_out_limit(t.ctx, 1) == 0 and t.L.zmi_ctx_set_scratch_limit(t.ctx, 64 << 20) == 0
    try:
        same(d0)
        n += 1
    finally:
        assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 8 << 30) == 0
        t.L.zmi_ctx_set_inflate_out_limit(t.ctx, 0)
    for shift in (1, 3, 15):
        d = t.directory(tiff, shift=shift)
        assert d.rec.tobytes() == d0.rec.tobytes() and d.info.tobytes() == d0.info.tobytes()
        same(d)
        n += 1
    for k in (0, 7, 19):
        one = t.read(d0, 0, sel=[k])
        assert (one.status, one.detail) == ([0], [0]) and bytes(one.slot(0)) == p.segs[k]
        n += 1
    return n


def arguments(t):
    tiff = Tiff([Page(20, 20, 3, 8, pred=2, tile=(16, 16), seed=71)])
    d = t.directory(tiff)
    assert t.directory(tiff, ctx=None).rc == E_ARG
    assert t.L.zmi_tiff_directory_dev(t.ctx, d.h_in.ptr, len(tiff.blob), d.h_pages.ptr, 1, None, t.mem.stream) == E_ARG
    assert t.L.zmi_tiff_directory_dev(t.ctx, None, len(tiff.blob), d.h_pages.ptr, 1, d.h_pages.ptr, t.mem.stream) == E_ARG
    assert t.L.zmi_tiff_directory_dev(t.ctx, d.h_in.ptr, len(tiff.blob), None, 1, d.h_pages.ptr, t.mem.stream) == E_ARG
    assert t.read(d, ctx=None).rc == E_ARG
    for align in (0, 3, 8192):
        assert t.read(d, align=align).rc == E_ARG
        check_read(t.read(d, align=align, flags=ASSEMBLE), tiff.pages[0], flags=ASSEMBLE)      # ignored there
    assert t.read(d, flags=2).rc == E_ARG
    assert t.read(d, null="off").rc == E_ARG
    assert t.read(d, null="st").rc == E_ARG
    assert t.read(d, null="det").rc == E_ARG
    zero = t.directory(tiff, cap=0)                                        # cap 0 counts
    assert zero.rc == 0 and int(zero.info["n_pages"]) == 1 and int(zero.info["n_listed"]) == 0 and int(zero.info["status"]) == 0
    check_read(t.read(d), tiff.pages[0])
    return 14
