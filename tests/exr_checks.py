"""Checks of the OpenEXR reader (zmi_exr_headers_dev / zmi_exr_read_dev, include/zmi355.h), shared by tests/test_emu_exr.py (CPU, the
emulator build) and tests/test_gpu_exr.py (the MI355X), both through the C ABI on buffers a `mem` object owns (put / full / read /
stream, as in tests/png_checks.py).

No OpenEXR library stands behind these tests: the judges are two pieces of code in this file, neither of them the code under test and
neither sharing code with the other -- the crafter `Exr` (struct.pack, a forward predictor and interleave written as loops over bytes,
zlib, the store-raw-when-not-smaller rule, placed faults) and the reference reader `read_exr` / `unzip` (a parser of its own, np.cumsum
and slicing).  tests/test_exr_craft.py pins both against the two byte-exact examples of the format's description and against each
other.  What a faulty zlib stream must report is judged by zlib.decompressobj.  ZMI_XE_SCRATCH is the one status no placed fault gives:
it reports the decoder's own Z_MEM_ERROR."""
import ctypes as C
import struct
import zlib

import numpy as np

Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR, Z_VERSION_ERROR, E_ARG = -3, -4, -5, -6, -103
(XE_MAGIC, XE_HEADER, XE_KIND, XE_COMPRESSION, XE_SAMPLING, XE_LEVELS, XE_CHANNELS, XE_BIG, XE_OUT, XE_SCRATCH, XE_CHUNK, XE_MISSING,
 XE_DATA, XE_LENGTH) = range(1, 15)
FLAG_STATUS = {XE_MAGIC: Z_DATA_ERROR, XE_HEADER: Z_DATA_ERROR, XE_KIND: Z_VERSION_ERROR, XE_COMPRESSION: Z_VERSION_ERROR,
               XE_SAMPLING: Z_VERSION_ERROR, XE_LEVELS: Z_VERSION_ERROR, XE_CHANNELS: Z_BUF_ERROR, XE_BIG: Z_VERSION_ERROR}
UINT, HALF, FLOAT = 0, 1, 2
NONE, RLE, ZIPS, ZIP, PIZ = 0, 1, 2, 3, 4
LINES = {0: 1, 1: 1, 2: 1, 3: 16, 4: 32, 5: 16, 6: 32, 7: 32, 8: 32, 9: 256}
SIZE = {UINT: 4, HALF: 2, FLOAT: 4}
NP = {UINT: "<u4", HALF: "<f2", FLOAT: "<f4"}
GUARD, FILL, CANARY = 64, 0xC7, 0x77
CHAN_CAP = 8
ATTRS_MAX = 65535
MAGIC = bytes.fromhex("762f3101")
IMAGE = np.dtype([("version", "<u4"), ("compression", "u1"), ("line_order", "u1"), ("tile_mode", "u1"), ("tiled", "u1"),
                  ("data_window", "<i4", 4), ("display_window", "<i4", 4), ("width", "<u4"), ("height", "<u4"), ("lines_per_chunk", "<u4"),
                  ("tile_w", "<u4"), ("tile_h", "<u4"), ("n_channels", "<u4"), ("n_chunks", "<u4"), ("row_bytes", "<u4"),
                  ("region_bytes", "<u4"), ("status", "<i4"), ("table_pos", "<u8")])
CHANNEL = np.dtype([("name_pos", "<u4"), ("name_len", "<u4"), ("pixel_type", "<i4"), ("x_sampling", "<i4"), ("y_sampling", "<i4"),
                    ("plane_off", "<u4")])
assert IMAGE.itemsize == 88 and CHANNEL.itemsize == 24
ONE_HALF = (("Y", HALF),)
RGBA = (("A", HALF), ("B", HALF), ("G", HALF), ("R", HALF))
MIXED = (("G", HALF), ("Z", FLOAT), ("id", UINT))
LAYOUTS = (ONE_HALF, RGBA, MIXED)


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.zmi_last_error.restype = C.c_char_p
    for f in (L.zmi_exr_trip, L.zmi_exr_piece):
        f.restype, f.argtypes = u32, []
    L.zmi_exr_headers_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp]
    L.zmi_exr_read_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, u32, u64, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    return L


# ---- the reference reader: a parser of its own, np.cumsum and slicing ------------------------------------------------------------------------
def unzip(d):
    """the inflated bytes of a ZIP / ZIPS chunk -> its raw bytes"""
    n = len(d)
    sums = np.cumsum(np.frombuffer(d, dtype=np.uint8).astype(np.int64)) - 128 * np.arange(n, dtype=np.int64)
    t = (sums % 256).astype(np.uint8)
    raw = np.empty(n, dtype=np.uint8)
    raw[0::2], raw[1::2] = t[:(n + 1) // 2], t[(n + 1) // 2:]
    return raw.tobytes()


def _cstr(blob, at):
    end = blob.index(b"\0", at)
    return blob[at:end], end + 1


def read_exr(blob, pad=0):
    """a good file -> dict(channels=[(name, type)], data_window, display_window, tiled, planes=[array [H, W]], region=bytes): the region
    as the contract lays it out, every plane at the next multiple of 4; pad = the bytes in front of such a plane, which no call writes"""
    assert blob[:4] == MAGIC
    version = struct.unpack_from("<I", blob, 4)[0]
    assert version & 0xFF == 2
    at, attrs = 8, {}
    while blob[at] != 0:
        name, at = _cstr(blob, at)
        _, at = _cstr(blob, at)
        size = struct.unpack_from("<i", blob, at)[0]
        attrs.setdefault(name, blob[at + 4:at + 4 + size])
        at += 4 + size
    table = at + 1
    channels, v, p = [], attrs[b"channels"], 0
    while v[p] != 0:
        name, p = _cstr(v, p)
        ptype, _, xs, ys = struct.unpack_from("<iIii", v, p)
        assert (xs, ys) == (1, 1)
        channels.append((name.decode(), ptype))
        p += 16
    comp = attrs[b"compression"][0]
    xmin, ymin, xmax, ymax = struct.unpack("<4i", attrs[b"dataWindow"])
    W, H = xmax - xmin + 1, ymax - ymin + 1
    tiled = bool(version & 0x200)
    boxes = []                                                            # (x0, y0, w, h) of chunk k, and its header's size
    if tiled:
        tw, th, mode = struct.unpack("<IIB", attrs[b"tiles"])
        assert mode & 15 == 0
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                boxes.append((x0, y0, min(tw, W - x0), min(th, H - y0)))
    else:
        step = LINES[comp]
        for y0 in range(0, H, step):
            boxes.append((0, y0, W, min(step, H - y0)))
    planes = [np.zeros((H, W), dtype=NP[t]) for _, t in channels]
    per_px = sum(SIZE[t] for _, t in channels)
    for k, (x0, y0, w, h) in enumerate(boxes):
        pos = struct.unpack_from("<Q", blob, table + 8 * k)[0]
        if tiled:
            tx, ty, lx, ly, size = struct.unpack_from("<5i", blob, pos)
            assert (tx * tw, ty * th, lx, ly) == (x0, y0, 0, 0)
            data = blob[pos + 20:pos + 20 + size]
        else:
            y, size = struct.unpack_from("<2i", blob, pos)
            assert y == ymin + y0
            data = blob[pos + 8:pos + 8 + size]
        n = w * h * per_px
        assert len(data) == size <= n
        raw = data if size == n else unzip(zlib.decompress(data))
        assert len(raw) == n
        rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, w * per_px)
        col = 0
        for c, (_, t) in enumerate(channels):
            run = w * SIZE[t]
            planes[c][y0:y0 + h, x0:x0 + w] = rows[:, col:col + run].copy().view(NP[t])
            col += run
    region = bytearray()
    for pl in planes:
        region += bytes([pad]) * (-len(region) % 4)
        region += pl.tobytes()
    return dict(channels=channels, data_window=(xmin, ymin, xmax, ymax), display_window=struct.unpack("<4i", attrs[b"displayWindow"]),
                tiled=tiled, planes=planes, region=bytes(region))


# ---- the crafter ------------------------------------------------------------------------------------------------------------------------------
def zip_forward(raw):
    """raw bytes of a chunk -> the bytes a ZIP / ZIPS writer hands to zlib (loops over bytes; the reference reader shares nothing with it)"""
    n = len(raw)
    t = bytearray(n)
    lo, hi = 0, (n + 1) // 2
    for i in range(n):
        if i % 2 == 0:
            t[lo] = raw[i]
            lo += 1
        else:
            t[hi] = raw[i]
            hi += 1
    d = bytearray(n)
    prev = 0
    for i in range(n):
        d[i] = t[i] if i == 0 else (t[i] - prev + 128) & 0xFF
        prev = t[i]
    return bytes(d)


def zip_forward_fast(raw):
    """the same bytes for large chunks; tests/test_exr_craft.py pins it against the loops"""
    a = np.frombuffer(raw, dtype=np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int16)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 0xFF
    return d.astype(np.uint8).tobytes()


def smooth_plane(ptype, W, H, seed):
    y, x = np.mgrid[0:H, 0:W]
    if ptype == HALF:
        return ((x * 3 + y * 5 + seed) % 2048 / 8.0).astype("<f2")
    if ptype == FLOAT:
        return (x * 0.5 + y * 1.25 + seed).astype("<f4")
    return ((x + y * W) * 3 + seed).astype("<u4")


def attr(name, type_, value):
    return name + b"\0" + type_ + b"\0" + struct.pack("<i", len(value)) + value


class Exr:
    """One crafted file.  channels: ((name, type), ..) in storage order; tile: (xSize, ySize) or None; order: the PHYSICAL order of the
    chunks -- 0 increasing, 1 decreasing, 2 shuffled -- written as lineOrder; noise: the chunks whose pixels are random bytes (they do not
    shrink, so they are stored raw); extra: [(position in the attribute list, attribute bytes)]; planes: the pixels, else smooth ramps.
    Faults: version (the word), drop (a set of attribute names), override (name -> attribute bytes), chlist (the value of `channels`),
    cut (the file's length), table (chunk -> entry), chunk_hdr (chunk -> header fields), stream (chunk -> the data bytes), comp_byte.
    flag = the record's status; expect = (status, detail) of a slot that reads the file; want = the region (from the reference reader; the padding in front of a plane, which stays
    untouched, as the FILL the tests lay under it)."""

    def __init__(self, width, height, channels=ONE_HALF, comp=ZIP, xmin=0, ymin=0, tile=None, order=0, noise=(), extra=(), seed=1, level=6,
                 planes=None, long_names=False, version=None, drop=(), override=None, chlist=None, cut=None, table=None, chunk_hdr=None,
                 stream=None, display=None, tile_mode=0, sampling=None, reference=True):
        self.width, self.height, self.channels, self.comp, self.tile = width, height, tuple(channels), comp, tile
        self.xmin, self.ymin = xmin, ymin
        self.window = (xmin, ymin, xmin + width - 1, ymin + height - 1)
        self.display = display or (0, 0, width - 1, height - 1)
        self.version = (2 | (0x200 if tile else 0) | (0x400 if long_names else 0)) if version is None else version
        self.lines = LINES[comp]
        self.per_px = sum(SIZE[t] for _, t in channels)
        self.row_bytes = width * self.per_px
        rng = np.random.RandomState(seed)
        if planes is None:
            planes = [smooth_plane(t, width, height, seed + 11 * c) for c, (_, t) in enumerate(channels)]
        self.planes = [np.ascontiguousarray(p, dtype=NP[t]) for p, (_, t) in zip(planes, channels)]
        if tile:
            self.boxes = [(x0, y0, min(tile[0], width - x0), min(tile[1], height - y0)) for y0 in range(0, height, tile[1])
                          for x0 in range(0, width, tile[0])]
            self.across = -(-width // tile[0])
        else:
            self.boxes = [(0, y0, width, min(self.lines, height - y0)) for y0 in range(0, height, self.lines)]
        self.n_chunks = len(self.boxes)
        for k in noise:
            x0, y0, w, h = self.boxes[k]
            for p, (_, t) in zip(self.planes, channels):
                junk = rng.randint(0, 256, (h, w * SIZE[t])).astype(np.uint8)
                p.view(np.uint8).reshape(height, width * SIZE[t])[y0:y0 + h, x0 * SIZE[t]:(x0 + w) * SIZE[t]] = junk
        # the header
        chl = b""
        for name, t in channels:
            xs, ys = (sampling or {}).get(name, (1, 1))
            chl += name.encode() + b"\0" + struct.pack("<iB3xii", t, 0, xs, ys)
        chl += b"\0"
        attrs = [(b"channels", attr(b"channels", b"chlist", chl if chlist is None else chlist)),
                 (b"compression", attr(b"compression", b"compression", bytes([comp]))),
                 (b"dataWindow", attr(b"dataWindow", b"box2i", struct.pack("<4i", *self.window))),
                 (b"displayWindow", attr(b"displayWindow", b"box2i", struct.pack("<4i", *self.display))),
                 (b"lineOrder", attr(b"lineOrder", b"lineOrder", bytes([order]))),
                 (b"pixelAspectRatio", attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))),
                 (b"screenWindowCenter", attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))),
                 (b"screenWindowWidth", attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)))]
        if tile:
            attrs.append((b"tiles", attr(b"tiles", b"tiledesc", struct.pack("<IIB", tile[0], tile[1], tile_mode))))
        attrs = [(n, (override or {}).get(n, a)) for n, a in attrs if n not in drop]
        parts = [a for _, a in attrs]
        for at, a in sorted(extra, key=lambda e: -e[0]):
            parts.insert(min(at, len(parts)), a)
        head = MAGIC + struct.pack("<I", self.version) + b"".join(parts) + b"\0"
        self.table_pos = len(head)
        # the chunks, in their physical order
        self.raw, self.data, self.stored = [], [], []
        for k, (x0, y0, w, h) in enumerate(self.boxes):
            rows = [p.view(np.uint8).reshape(height, width * SIZE[t])[y0:y0 + h, x0 * SIZE[t]:(x0 + w) * SIZE[t]]
                    for p, (_, t) in zip(self.planes, channels)]
            raw = np.concatenate(rows, axis=1).tobytes() if rows else b""
            self.raw.append(raw)
            data = raw
            if comp in (ZIPS, ZIP):
                packed = zlib.compress(zip_forward_fast(raw) if len(raw) > 4096 else zip_forward(raw), level)
                if len(packed) < len(raw):
                    data = packed
            data = (stream or {}).get(k, data)
            self.data.append(data)
            self.stored.append(len(data) == len(raw))
        phys = list(range(self.n_chunks))
        if order == 1:
            phys.reverse()
        elif order == 2:
            rng.shuffle(phys)
        self.phys = phys
        body, entries, at = bytearray(), [0] * self.n_chunks, self.table_pos + 8 * self.n_chunks
        for k in phys:
            x0, y0, w, h = self.boxes[k]
            f = dict(y=ymin + y0, tx=x0 // tile[0] if tile else 0, ty=y0 // tile[1] if tile else 0, lx=0, ly=0, size=len(self.data[k]))
            f.update((chunk_hdr or {}).get(k, {}))
            hdr = struct.pack("<5i", f["tx"], f["ty"], f["lx"], f["ly"], f["size"]) if tile else struct.pack("<2i", f["y"], f["size"])
            entries[k] = at + len(body)
            body += hdr + self.data[k]
        for k, e in (table or {}).items():
            entries[k] = e
        self.blob = (head + struct.pack("<%dQ" % self.n_chunks, *entries) + bytes(body))[:cut]
        self.plane_off, off = [], 0
        for _, t in channels:
            off += -off % 4
            self.plane_off.append(off)
            off += width * height * SIZE[t]
        self.region_bytes = off
        self.flag, self.expect = 0, (0, 0)
        self.want = None
        if reference:
            ref = read_exr(self.blob, FILL)
            assert ref["channels"] == [(n, t) for n, t in channels] and ref["data_window"] == self.window and ref["tiled"] == bool(tile)
            for got, p in zip(ref["planes"], self.planes):
                assert got.tobytes() == p.tobytes()                       # the crafter's forward transform against the reference reader
            self.want = ref["region"]
            assert len(self.want) == self.region_bytes

    def flagged(self, code):
        self.flag, self.expect = code, (FLAG_STATUS[code], code)
        return self

    def fails(self, code, chunk=0, status=Z_DATA_ERROR):
        self.expect = (status, code | chunk << 8)
        return self


def judge_stream(payload, n):
    """what zlib says of a stream that must give exactly n bytes"""
    d = zlib.decompressobj()
    try:
        raw = d.decompress(payload, n + 1)
    except zlib.error:
        return XE_DATA
    return XE_LENGTH if len(raw) != n or not d.eof else 0


# ---- the target -------------------------------------------------------------------------------------------------------------------------------
class Batch:
    def __init__(self, rc, rec, chans, h_in, h_off, h_len, h_img, h_ch, n, files, cap):
        self.rc, self.rec, self.chans, self.h_in, self.h_off, self.h_len, self.h_img, self.h_ch = rc, rec, chans, h_in, h_off, h_len, h_img, h_ch
        self.n, self.files, self.cap = n, files, cap


class Read:
    def __init__(self, rc, off, length, status, detail, out, clean):
        self.rc, self.off, self.len, self.status, self.detail, self.out, self.clean = rc, off, length, status, detail, out, clean

    def slot(self, j):
        return self.out[self.off[j]:self.off[j] + self.len[j]]


def plan(rec, sel, n_sel, align):
    """the contract's offsets and bounds from the host copy of the records: (offsets + [need], sizes, chunks, raw bytes)"""
    off, sizes, at, chunks, raw = [], [], 0, 0, 0
    align = align if 1 <= align <= 4096 and not align & (align - 1) else 1
    for j in range(n_sel):
        k = j if sel is None else sel[j]
        ok = k < len(rec) and int(rec[k]["status"]) == 0
        size = int(rec[k]["region_bytes"]) if ok else 0
        if ok:
            chunks += int(rec[k]["n_chunks"])
            raw += int(rec[k]["height"]) * int(rec[k]["row_bytes"])
        off.append(at)
        sizes.append(size)
        at += -(-size // align) * align
    return off + [at], sizes, chunks, raw


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.trip, self.piece = int(self.L.zmi_exr_trip()), int(self.L.zmi_exr_piece())

    def headers(self, files, shift=0, gap=0, chan_cap=CHAN_CAP, ctx="ctx"):
        """one zmi_exr_headers_dev call on the files laid out one behind the other, `gap` bytes of 0xEE between them; a record of canary
        stands behind either table"""
        m, n = self.mem, len(files)
        blob, offs = bytearray(), []
        for k, p in enumerate(files):
            blob += b"\xEE" * (gap + (k * 5 % 7 if gap else 0))
            offs.append(len(blob))
            blob += p.blob
        h_in = m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift)
        h_off = m.put(np.array(offs + [0], dtype=np.uint64))
        h_len = m.put(np.array([len(p.blob) for p in files] + [0], dtype=np.uint32))
        h_img = m.full((n + 1) * 88, CANARY)
        h_ch = m.full((n * chan_cap + 1) * 24, CANARY)
        rc = self.L.zmi_exr_headers_dev(self.ctx if ctx == "ctx" else ctx, h_in.ptr, h_off.ptr, h_len.ptr, n, h_img.ptr, h_ch.ptr, chan_cap, m.stream)
        if rc != 0:
            return Batch(rc, None, None, h_in, h_off, h_len, h_img, h_ch, n, files, chan_cap)
        rec, ch = m.read(h_img, IMAGE), m.read(h_ch, CHANNEL)
        assert rec[n:].tobytes() == bytes([CANARY]) * 88 and ch[n * chan_cap:].tobytes() == bytes([CANARY]) * 24, "the call wrote behind its tables"
        return Batch(rc, rec[:n], ch[:n * chan_cap].reshape(n, chan_cap), h_in, h_off, h_len, h_img, h_ch, n, files, chan_cap)

    def read(self, b, sel=None, n_sel=None, align=1, cap=None, n_files=None, chunk_cap=None, decoded=None, flags=0, null=None, ctx="ctx"):
        """one zmi_exr_read_dev call on the batch; cap / chunk_cap / decoded None: exactly what the selection needs"""
        m = self.mem
        n_files = b.n if n_files is None else n_files
        if n_sel is None:
            n_sel = n_files if sel is None else len(sel)
        plan_off, plan_size, chunks, raw = plan(b.rec[:n_files], sel, n_sel, align)
        need = plan_off[-1]
        cap = need if cap is None else cap
        chunk_cap = chunks if chunk_cap is None else chunk_cap
        decoded = raw if decoded is None else decoded
        h_sel = m.put(np.array(list(sel) + [0], dtype=np.uint32)) if sel is not None else None
        h_out = m.full(GUARD + cap + GUARD, FILL)
        h_o = m.full((n_sel + 2) * 8, CANARY)
        h_l = m.full((n_sel + 1) * 4, CANARY)
        h_s = m.full((n_sel + 1) * 4, CANARY)
        h_d = m.full((n_sel + 1) * 4, CANARY)
        args = dict(off=h_o.ptr, len=h_l.ptr, st=h_s.ptr, det=h_d.ptr)
        if null:
            args[null] = None
        rc = self.L.zmi_exr_read_dev(self.ctx if ctx == "ctx" else ctx, b.h_in.ptr, b.h_off.ptr, b.h_len.ptr, b.h_img.ptr, b.h_ch.ptr, b.cap,
                                     n_files, h_sel.ptr if h_sel else None, n_sel, chunk_cap, decoded, flags, align, h_out.ptr + GUARD, cap,
                                     args["off"], args["len"], args["st"], args["det"], m.stream)
        if rc != 0:
            return Read(rc, None, None, None, None, None, True)
        off = [int(x) for x in m.read(h_o, np.uint64)]
        ln = [int(x) for x in m.read(h_l, np.uint32)]
        st = [int(x) for x in m.read(h_s, np.int32)]
        det = [int(x) for x in m.read(h_d, np.int32)]
        buf = m.read(h_out, np.uint8)
        word = int.from_bytes(bytes([CANARY]) * 8, "little")
        assert off[n_sel + 1] == word and ln[n_sel] == word & 0xFFFFFFFF, "the call wrote behind its tables"
        touched = np.zeros(cap, dtype=bool)
        for j in range(n_sel):
            if plan_off[j] + plan_size[j] <= cap:
                touched[plan_off[j]:plan_off[j] + plan_size[j]] = True
        body = buf[GUARD:GUARD + cap]
        clean = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all() and (body[~touched] == FILL).all())
        r = Read(rc, off[:n_sel + 1], ln[:n_sel], st[:n_sel], det[:n_sel], body.tobytes(), clean)
        r.plan_off, r.need = plan_off, need
        return r


# ---- judges -----------------------------------------------------------------------------------------------------------------------------------
def check_records(b):
    """every record and channel record against what the crafter wrote"""
    assert b.rc == 0
    for k, (e, p) in enumerate(zip(b.rec, b.files)):
        assert int(e["status"]) == p.flag, (k, int(e["status"]), p.flag)
        if p.flag in (XE_MAGIC, XE_HEADER):
            continue
        got = (int(e["version"]), int(e["compression"]), tuple(int(x) for x in e["data_window"]), tuple(int(x) for x in e["display_window"]),
               int(e["n_channels"]), int(e["tiled"]), int(e["lines_per_chunk"]))
        assert got == (p.version, p.comp, p.window, p.display, len(p.channels), 1 if p.tile else 0, LINES[p.comp]), (k, got)
        if p.flag == XE_BIG:
            continue
        assert (int(e["width"]), int(e["height"])) == (p.width, p.height), k
        assert (int(e["tile_w"]), int(e["tile_h"])) == (tuple(p.tile) if p.tile else (0, 0)), k
        for c, (name, t) in enumerate(p.channels[:b.cap]):
            ch = b.chans[k][c]
            at = int(ch["name_pos"])
            assert p.blob[at:at + int(ch["name_len"])] == name.encode() and int(ch["pixel_type"]) == t, (k, c)
        if p.flag in (0, XE_COMPRESSION, XE_KIND):
            assert (int(e["row_bytes"]), int(e["region_bytes"]), int(e["table_pos"])) == (p.row_bytes, p.region_bytes, p.table_pos), k
            assert [int(b.chans[k][c]["plane_off"]) for c in range(len(p.channels))] == p.plane_off, k
        if p.flag == 0:
            assert int(e["n_chunks"]) == p.n_chunks, k
            assert b.chans[k][len(p.channels):].tobytes() == bytes(24 * (b.cap - len(p.channels))), k


def check_read(r, files, sel=None):
    """every slot's words and bytes, the offsets, the need, and nothing written elsewhere"""
    assert r.rc == 0 and r.clean, (r.rc, r.clean)
    assert r.off == r.plan_off, (r.off[:8], r.plan_off[:8])
    for j in range(len(r.status)):
        k = j if sel is None else sel[j]
        st, det = files[k].expect if k < len(files) else (E_ARG, 0)
        assert (r.status[j], r.detail[j]) == (st, det), (j, k, r.status[j], r.detail[j], st, det)
        if st == 0:
            want = files[k].want
            assert r.len[j] == len(want), (j, k, r.len[j], len(want))
            got = r.slot(j)
            if got != want:
                bad = next(i for i in range(len(want)) if got[i] != want[i])
                raise AssertionError("slot %d file %d (%d x %d, %s, compression %d): byte %d of the region is %d, not %d"
                                     % (j, k, files[k].width, files[k].height, files[k].channels, files[k].comp, bad, got[bad], want[bad]))
        else:
            assert r.len[j] == 0, (j, k)


def run(t, files, shift=0, align=1, gap=0, sel=None, chan_cap=CHAN_CAP):
    """headers and read of a batch, everything checked"""
    b = t.headers(files, shift=shift, gap=gap, chan_cap=chan_cap)
    check_records(b)
    r = t.read(b, sel=sel, align=align)
    check_read(r, files, sel=sel)
    return b, r


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------------------
def geometry(t, widths=(1, 2, 3, 5, 17, 63, 64, 65, 257), heights=(1, 15, 16, 17, 33), comps=(ZIPS, ZIP, NONE), layouts=LAYOUTS):
    """every width x height x compression x channel layout: h even and odd, runs shorter than a lane's 16 bytes, a short last chunk"""
    n = 0
    for li, layout in enumerate(layouts):
        for comp in comps:
            files = [Exr(w, h, layout, comp, seed=w + 3 * h + li) for h in heights for w in widths]
            run(t, files, align=16, shift=li)
            n += len(files)
    return n


def trips(t, comps=(ZIPS, ZIP)):
    """run lengths at a trip's and at a piece's size - 2, + 0, + 2 bytes in HALF pixels; the same around the trip in FLOAT pixels (- 4, + 0,
    + 4) next to a HALF channel, which makes the second run start at an odd multiple of 2"""
    T, P = t.trip, t.piece
    files = []
    for comp in comps:
        for size in (T - 2, T, T + 2, P - 2, P, P + 2, 2 * P + 2):
            files.append(Exr(size // 2, 3, ONE_HALF, comp, seed=size))
        for size in (T - 4, T, T + 4):
            files.append(Exr(size // 4, 2, (("A", HALF), ("Z", FLOAT)), comp, seed=size + 1))
    run(t, files, align=4)
    return len(files)


def carries(t, width=4099, rows=16):
    """one chunk of 16 x 4099 RGBA HALF (524 KiB): it crosses many blocks and trips, and the byte sums of its blocks are not 0 mod 256"""
    p = Exr(width, rows, RGBA, ZIP, seed=7, level=1)
    assert p.n_chunks == 1 and not p.stored[0]
    d = np.frombuffer(zlib.decompress(p.data[0]), dtype=np.uint8)
    sums = [int(d[at:at + 1024].sum()) % 256 for at in range(0, len(d), 1024)]
    assert sum(s != 0 for s in sums) > len(sums) // 2
    run(t, [p], align=16)
    return 1


def raw_chunks(t):
    """smooth data for compressed chunks and noise for raw-stored ones in the same file, scanlines and tiles, and a file of noise only"""
    a = Exr(70, 50, RGBA, ZIP, noise=(1, 3), seed=3)
    b = Exr(33, 9, MIXED, ZIPS, noise=(0, 4, 8), seed=4)
    c = Exr(37, 21, ONE_HALF, ZIP, tile=(16, 16), noise=(2, 5), order=2, seed=5)
    d = Exr(19, 20, RGBA, ZIP, noise=(0, 1), seed=6)
    assert a.stored == [False, True, False, True] and c.stored.count(True) == 2 and all(d.stored) and b.stored.count(True) == 3
    for shift in (0, 1):
        run(t, [a, b, c, d], align=16, shift=shift)
    return 4


def tiles(t, sizes=((16, 16), (32, 8))):
    """tiles of 16 x 16 and 32 x 8 on 37 x 21 and on exactly one tile, chunks physically shuffled, ZIP and NONE, windows off the origin"""
    files = []
    for tw, th in sizes:
        for comp in (ZIP, NONE):
            files.append(Exr(37, 21, RGBA, comp, tile=(tw, th), order=2, seed=tw + comp, xmin=-5, ymin=3))
            files.append(Exr(tw, th, MIXED, comp, tile=(tw, th), order=2, seed=th + comp))
            files.append(Exr(2 * tw, 3 * th, ONE_HALF, comp, tile=(tw, th), order=1, seed=th))
    run(t, files, align=16)
    return len(files)


def layout(t):
    """the three line orders as physical orders, windows with negative corners, long names, unknown attributes in every position, a
    channel list that is not sorted, a second displayWindow, 65 535 attributes, nine channels under a chan_cap of 9"""
    unknown = attr(b"owner", b"string", b"somebody") + attr(b"chromaticities", b"chromaticities", struct.pack("<8f", *range(8)))
    empty = attr(b"comments", b"string", b"")
    files = [Exr(21, 40, RGBA, ZIP, order=0, seed=1), Exr(21, 40, RGBA, ZIP, order=1, seed=2), Exr(21, 40, RGBA, ZIPS, order=1, seed=3),
             Exr(40, 33, MIXED, ZIP, tile=(16, 16), order=2, seed=4), Exr(9, 20, MIXED, ZIP, xmin=-4, ymin=-30, seed=5),
             Exr(9, 20, ONE_HALF, ZIPS, xmin=-100, ymin=-7, display=(-5, -5, 80, 60), seed=6),
             Exr(12, 18, (("a channel with a name of more than 31 bytes", HALF), ("b", FLOAT)), ZIP, long_names=True, seed=7),
             Exr(12, 18, (("Z", FLOAT), ("A", HALF), ("id", UINT), ("B", HALF)), ZIP, seed=8)]
    for at in range(10):
        files.append(Exr(11, 17, MIXED, ZIP, extra=[(at, unknown), (at, empty)], seed=10 + at))
    files.append(Exr(11, 17, MIXED, ZIP, tile=(8, 8), extra=[(9, unknown)], seed=30))
    # an attribute that stands twice: the first counts; exactly the most attributes a header may have
    files.append(Exr(11, 17, MIXED, ZIP, seed=31, extra=[(8, attr(b"displayWindow", b"box2i", struct.pack("<4i", 1, 2, 3, 4)))]))
    files.append(Exr(11, 17, MIXED, ZIP, seed=32, extra=[(3, attr(b"x", b"int", bytes(4)) * (ATTRS_MAX - 8))]))
    run(t, files, align=16, shift=3)
    nine = Exr(7, 5, tuple(("c%d" % k, (HALF, FLOAT, UINT)[k % 3]) for k in range(9)), ZIP, seed=9)
    run(t, [nine, files[0]], chan_cap=9)
    return len(files) + 1


# ---- 2. every status code, among good neighbours ----------------------------------------------------------------------------------------------
def header_faults():
    """-> [(name, Exr)]: every status of the headers call"""
    def base(**kw):
        args = dict(channels=MIXED, comp=ZIP, seed=21, reference=False)
        args.update(kw)
        return Exr(10, 20, **args)

    good = base()
    cases = []
    bad = base()
    bad.blob = b"\x76\x2f\x31\x02" + bad.blob[4:]
    cases.append(("magic", bad.flagged(XE_MAGIC)))
    short = base()
    short.blob = short.blob[:7]
    cases.append(("seven bytes", short.flagged(XE_MAGIC)))
    H = XE_HEADER
    cases.append(("version 1", base(version=1).flagged(H)))
    cases.append(("attribute leaves the file", base(cut=good.table_pos - 20).flagged(H)))
    cases.append(("name leaves the file", base(cut=12).flagged(H)))
    cases.append(("name of 32 bytes", base(extra=[(2, attr(b"n" * 32, b"int", bytes(4)))]).flagged(H)))
    cases.append(("name of 256 bytes", base(long_names=True, extra=[(2, attr(b"n" * 256, b"int", bytes(4)))]).flagged(H)))
    cases.append(("empty type name", base(extra=[(3, attr(b"thing", b"", bytes(4)))]).flagged(H)))
    cases.append(("negative size", base(extra=[(1, b"thing\0int\0" + struct.pack("<i", -4))]).flagged(H)))
    for name in (b"channels", b"compression", b"dataWindow", b"lineOrder"):
        cases.append(("no " + name.decode(), base(drop={name}).flagged(H)))
    cases.append(("tiled without tiles", base(tile=(8, 8), drop={b"tiles"}).flagged(H)))
    cases.append(("compression of 2 bytes", base(override={b"compression": attr(b"compression", b"compression", b"\3\0")}).flagged(H)))
    cases.append(("dataWindow of 12 bytes", base(override={b"dataWindow": attr(b"dataWindow", b"box2i", bytes(12))}).flagged(H)))
    cases.append(("tiles of 8 bytes", base(tile=(8, 8), override={b"tiles": attr(b"tiles", b"tiledesc", bytes(8))}).flagged(H)))
    cases.append(("inverted window", base(override={b"dataWindow": attr(b"dataWindow", b"box2i", struct.pack("<4i", 5, 0, 4, 19))}).flagged(H)))
    one = b"G\0" + struct.pack("<iB3xii", 1, 0, 1, 1)
    cases.append(("pixel type 3", base(chlist=b"G\0" + struct.pack("<iB3xii", 3, 0, 1, 1) + b"\0").flagged(H)))
    cases.append(("zero channels", base(chlist=b"\0").flagged(H)))
    cases.append(("sampling 0", base(chlist=b"G\0" + struct.pack("<iB3xii", 1, 0, 0, 1) + b"\0").flagged(H)))
    cases.append(("channel list without its end", base(chlist=one).flagged(H)))
    cases.append(("channel list with bytes behind its end", base(chlist=one + b"\0\0").flagged(H)))
    cases.append(("compression 10", base(override={b"compression": attr(b"compression", b"compression", b"\x0a")}).flagged(H)))
    cases.append(("line order 3", base(override={b"lineOrder": attr(b"lineOrder", b"lineOrder", b"\3")}).flagged(H)))
    cases.append(("tile size 0", base(tile=(8, 8), override={b"tiles": attr(b"tiles", b"tiledesc", struct.pack("<IIB", 0, 8, 0))}).flagged(H)))
    cases.append(("offset table leaves the file", base(cut=good.table_pos + 8 * good.n_chunks - 1).flagged(H)))
    cases.append(("no end of the header", base(cut=good.table_pos - 1).flagged(H)))
    cases.append(("one attribute too many", base(extra=[(3, attr(b"x", b"int", bytes(4)) * (ATTRS_MAX - 7))]).flagged(H)))
    cases.append(("deep", base(version=2 | 0x800).flagged(XE_KIND)))
    cases.append(("multi-part", base(version=2 | 0x1000).flagged(XE_KIND)))
    for comp in (RLE, PIZ, 9):
        p = base(comp=NONE, override={b"compression": attr(b"compression", b"compression", bytes([comp]))})
        p.comp = comp
        cases.append(("compression %d" % comp, p.flagged(XE_COMPRESSION)))
    cases.append(("sampling 2", base(sampling={"Z": (2, 2)}).flagged(XE_SAMPLING)))
    cases.append(("mipmap", base(tile=(8, 8), tile_mode=1).flagged(XE_LEVELS)))
    cases.append(("ripmap, rounding up", base(tile=(8, 8), tile_mode=0x12).flagged(XE_LEVELS)))
    many = Exr(4, 4, tuple(("c%02d" % k, HALF) for k in range(CHAN_CAP + 1)), ZIP, seed=3, reference=False)
    cases.append(("nine channels", many.flagged(XE_CHANNELS)))
    big = base(override={b"dataWindow": attr(b"dataWindow", b"box2i", struct.pack("<4i", 0, 0, 0x7FFFFFFE, 1))})
    big.window = (0, 0, 0x7FFFFFFE, 1)
    cases.append(("a region of 2^33 bytes", big.flagged(XE_BIG)))
    big2 = Exr(10, 20, ONE_HALF, ZIP, seed=1, reference=False,
               override={b"dataWindow": attr(b"dataWindow", b"box2i", struct.pack("<4i", -0x80000000, 0, 0x7FFFFFFF, 1))})
    big2.window = (-0x80000000, 0, 0x7FFFFFFF, 1)
    cases.append(("a width of 2^32", big2.flagged(XE_BIG)))
    return cases


def chunk_faults():
    """-> [(name, Exr)]: every status a chunk gives a slot"""
    def base(**kw):
        args = dict(channels=MIXED, comp=ZIP, seed=21, reference=False)
        args.update(kw)
        return Exr(10, 40, **args)

    def tiled(**kw):
        return base(tile=(8, 16), **kw)

    good = base()
    n = len(good.raw[1])
    d = zip_forward(good.raw[1])
    size = len(good.blob)
    cases = []
    cases.append(("table entry behind the file", base(table={2: size}).fails(XE_CHUNK, 2)))
    cases.append(("chunk header leaves the file", base(table={1: size - 7}).fails(XE_CHUNK, 1)))
    cases.append(("table entry of 2^63", base(table={0: 1 << 63}).fails(XE_CHUNK, 0)))
    cases.append(("wrong y", base(chunk_hdr={1: dict(y=15)}).fails(XE_CHUNK, 1)))
    cases.append(("y of another window", base(ymin=-8, chunk_hdr={2: dict(y=32)}).fails(XE_CHUNK, 2)))
    cases.append(("wrong tile x", tiled(chunk_hdr={3: dict(tx=0)}).fails(XE_CHUNK, 3)))
    cases.append(("wrong tile y", tiled(chunk_hdr={0: dict(ty=1)}).fails(XE_CHUNK, 0)))
    cases.append(("level 1", tiled(chunk_hdr={1: dict(lx=1)}).fails(XE_CHUNK, 1)))
    cases.append(("level y 1", tiled(chunk_hdr={1: dict(ly=1)}).fails(XE_CHUNK, 1)))
    cases.append(("negative dataSize", base(chunk_hdr={1: dict(size=-1)}).fails(XE_CHUNK, 1)))
    cases.append(("dataSize above n", base(chunk_hdr={0: dict(size=n + 1)}).fails(XE_CHUNK, 0)))
    last = base(order=0)
    cases.append(("data leaves the file", base(cut=size - 1).fails(XE_CHUNK, last.n_chunks - 1)))
    cases.append(("NONE with a short chunk", base(comp=NONE, chunk_hdr={1: dict(size=n - 2)}).fails(XE_CHUNK, 1)))
    cases.append(("two bad chunks: the first counts", base(chunk_hdr={2: dict(y=0), 1: dict(size=-5)}).fails(XE_CHUNK, 1)))
    cases.append(("missing", base(table={2: 0}).fails(XE_MISSING, 2)))
    cases.append(("chunk before missing", base(table={0: 0}, chunk_hdr={2: dict(y=1)}).fails(XE_CHUNK, 2)))
    stream = zlib.compress(d)
    adler = stream[:-4] + struct.pack(">I", zlib.adler32(d) ^ 1)
    assert judge_stream(adler, n) == XE_DATA
    cases.append(("adler", base(stream={1: adler}).fails(XE_DATA, 1)))
    bad = bytearray(stream)
    bad[len(bad) // 2] ^= 0x10
    cases.append(("corrupt", base(stream={1: bytes(bad)}).fails(judge_stream(bytes(bad), n), 1)))
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, b"a preset dictionary")
    fdict = z.compress(d) + z.flush()
    assert fdict[1] & 0x20
    cases.append(("fdict", base(stream={2: fdict}).fails(XE_DATA, 2)))
    cases.append(("missing before data", base(table={2: 0}, stream={1: adler}).fails(XE_MISSING, 2)))
    cases.append(("two bytes short", base(stream={1: zlib.compress(d[:-2])}).fails(XE_LENGTH, 1)))
    cases.append(("two bytes long", base(stream={1: zlib.compress(d + b"\x80\x80")}).fails(XE_LENGTH, 1)))
    cases.append(("cut stream", base(stream={0: zlib.compress(zip_forward(good.raw[0]))[:40]}).fails(XE_LENGTH, 0)))
    cases.append(("one byte", base(stream={1: stream[:1]}).fails(XE_LENGTH, 1)))
    cases.append(("data before length", base(stream={2: zlib.compress(zip_forward(good.raw[2])[:-2]), 1: adler}).fails(XE_DATA, 1)))
    junk = base(stream={1: stream + b"junk"})                                # bytes behind the stream, inside dataSize: accepted
    junk.want = good_region(good)
    cases.append(("junk behind the stream", junk))
    return cases


def good_region(p):
    return read_exr(p.blob, FILL)["region"]


def statuses(t):
    """each fault as file 1 of three, the neighbours still reading right; then all of them in one batch"""
    cases = header_faults() + chunk_faults()
    left, right = Exr(8, 35, RGBA, ZIP, seed=31), Exr(33, 5, MIXED, ZIPS, tile=(16, 4), seed=32)
    seen = set()
    for name, p in cases:
        try:
            run(t, [left, p, right], align=16)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        seen.add(p.expect[1] & 0xFF)
    assert seen == set(range(0, XE_LENGTH + 1)) - {XE_OUT, XE_SCRATCH}, sorted(seen)
    run(t, [left] + [p for _, p in cases] + [right])
    return len(cases)


# ---- 3. selection and room --------------------------------------------------------------------------------------------------------------------
def mixed(n, seed=0):
    """n files of mixed shapes, layouts and compressions, a few tiled"""
    files = []
    for i in range(n):
        w, h = 1 + (i * 7 + seed) % 23, 1 + (i * 5 + seed * 3) % 37
        tile = (8, 8) if i % 5 == 3 else None
        files.append(Exr(w, h, LAYOUTS[(i + seed) % 3], (ZIP, ZIPS, NONE)[i % 3], tile=tile, order=2 if tile else i % 2, seed=i + 1,
                         xmin=-(i % 4), ymin=i % 3 - 1))
    return files


def selection(t):
    """selections with duplicates and bad indices, n_sel 0; out_cap exact, one byte short, cut behind the second file, 0; chunk_cap and
    decoded_bytes exact and one too small"""
    files = mixed(7)
    files[4] = [p for name, p in header_faults() if name == "compression 4"][0]
    b = t.headers(files)
    check_records(b)
    n = 0
    for sel in ([1, 3, 5], [6, 5, 4, 3, 2, 1, 0], [2, 2, 0, 2], [0, 7, 1, 4000000000, 2], []):
        for align in (1, 16):
            r = t.read(b, sel=sel, align=align)
            if sel:
                check_read(r, files, sel=sel)
            else:
                assert r.rc == 0 and r.off == [0] and r.clean
            n += 1
    full = t.read(b, align=16)
    check_read(full, files)
    need, end2 = full.need, full.off[1] + len(files[1].want)
    for cap in (need, need - 1, end2, 0):
        r = t.read(b, align=16, cap=cap)
        assert r.rc == 0 and r.clean and r.off == full.off and r.off[-1] == need
        for j, p in enumerate(files):
            if p.flag:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_VERSION_ERROR, XE_COMPRESSION, 0)
            elif r.off[j] + len(p.want) <= cap:
                assert (r.status[j], r.detail[j], r.len[j]) == (0, 0, len(p.want)) and r.slot(j) == p.want, (cap, j)
            else:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_BUF_ERROR, XE_OUT, 0), (cap, j)
        n += 1
    _, _, chunks, raw = plan(b.rec, None, len(files), 16)
    last = len(files) - 1
    for kw in (dict(chunk_cap=chunks - 1), dict(decoded=raw - 1), dict(chunk_cap=files[0].n_chunks), dict(decoded=0), dict(chunk_cap=0)):
        r = t.read(b, align=16, **kw)
        assert r.rc == 0 and r.clean and r.off == full.off
        fits_c, fits_r = 0, 0
        for j, p in enumerate(files):
            if p.flag:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_VERSION_ERROR, XE_COMPRESSION, 0)
                continue
            fits_c += p.n_chunks
            fits_r += p.height * p.row_bytes
            if fits_c <= kw.get("chunk_cap", chunks) and fits_r <= kw.get("decoded", raw):
                assert (r.status[j], r.detail[j]) == (0, 0) and r.slot(j) == p.want, (kw, j)
            else:
                assert (r.status[j], r.detail[j], r.len[j]) == (E_ARG, 0, 0), (kw, j)
        assert r.status[last] == E_ARG
        n += 1
    return n


def forged_record(t):
    """a record no headers call would write for its file is ZMI_E_ARG in the slot, takes no room and nothing of it is read; the neighbours
    read right"""
    files = [Exr(9, 20, MIXED, ZIP, seed=1), Exr(21, 35, MIXED, ZIP, seed=2), Exr(20, 20, RGBA, ZIP, tile=(8, 8), seed=3)]
    b = t.headers(files)
    size = len(files[1].blob)
    forged = [("width", 22), ("height", 36), ("n_chunks", 4), ("n_chunks", 2), ("row_bytes", 212), ("region_bytes", 1 << 20), ("table_pos", size - 8),
              ("table_pos", 0), ("lines_per_chunk", 1), ("compression", 2), ("compression", 4), ("tiled", 1), ("tile_w", 8), ("version", 2 | 0x200),
              ("version", 2 | 0x1000), ("n_channels", 2), ("n_channels", CHAN_CAP + 1), ("n_channels", 0), ("data_window", (0, 0, 21, 34)),
              ("status", -7)]
    n = 0
    for field, value in forged:
        rec = b.rec.copy()
        rec[1][field] = value
        n += _forged(t, b, files, rec, b.chans, field)
    for field, value in (("plane_off", 4), ("pixel_type", 2), ("pixel_type", 3), ("x_sampling", 2)):
        ch = b.chans.copy()
        ch[1][0][field] = value
        n += _forged(t, b, files, b.rec.copy(), ch, field)
    return n


def _forged(t, b, files, rec, ch, what):
    fb = Batch(0, rec.copy(), ch, b.h_in, b.h_off, b.h_len, t.mem.put(rec), t.mem.put(ch), b.n, files, b.cap)
    fb.rec[1]["status"] = -1                                              # (for the plan of this file: the slot takes no room)
    r = t.read(fb, align=16)
    assert r.rc == 0 and r.clean and r.off == r.plan_off, what
    assert (r.status[1], r.detail[1], r.len[1]) == (E_ARG, 0, 0), (what, r.status[1], r.detail[1])
    for j in (0, 2):
        assert (r.status[j], r.detail[j]) == (0, 0) and r.slot(j) == files[j].want, (what, j)
    return 1


# ---- 4. independence, arguments ---------------------------------------------------------------------------------------------------------------
def independence(t, count=12):
    """the same words and bytes at input alignments 0 .. 3 and 15, with gaps between the files, in another slot order, with other files
    in the table, and alone"""
    files = mixed(count)
    b0 = t.headers(files)
    ref = t.read(b0, align=16)
    check_read(ref, files)
    n = 1
    for shift in (1, 2, 3, 15):
        b = t.headers(files, shift=shift, gap=shift)
        assert b.rec["status"].tolist() == b0.rec["status"].tolist() and b.rec["table_pos"].tolist() == b0.rec["table_pos"].tolist()
        r = t.read(b, align=16)
        assert (r.off, r.len, r.status, r.detail, r.out) == (ref.off, ref.len, ref.status, ref.detail, ref.out), shift
        n += 1
    order = list(range(count))[::-1]
    r = t.read(b0, sel=order, align=16)
    check_read(r, files, sel=order)
    for j, k in enumerate(order):
        assert r.slot(j) == ref.slot(k)
    n += 1
    for k in (0, 3, count - 1):
        one = t.read(b0, sel=[k])
        assert (one.status, one.detail) == ([0], [0]) and one.slot(0) == files[k].want
        alone = t.read(t.headers([files[k]]))
        assert alone.status == [0] and alone.slot(0) == files[k].want
        n += 1
    return n


def arguments(t):
    files = mixed(3)
    b = t.headers(files)
    assert t.headers(files, ctx=None).rc == E_ARG
    assert t.read(b, ctx=None).rc == E_ARG
    for align in (0, 3, 8192):
        assert t.read(b, align=align).rc == E_ARG
    assert t.read(b, flags=1).rc == E_ARG
    assert t.read(b, null="off").rc == E_ARG
    assert t.read(b, null="st").rc == E_ARG
    assert t.read(b, null="det").rc == E_ARG
    assert t.read(b, chunk_cap=1 << 31).rc == E_ARG
    assert t.L.zmi_exr_headers_dev(t.ctx, b.h_in.ptr, None, b.h_len.ptr, 3, b.h_img.ptr, b.h_ch.ptr, b.cap, t.mem.stream) == E_ARG
    assert t.L.zmi_exr_headers_dev(t.ctx, b.h_in.ptr, b.h_off.ptr, b.h_len.ptr, 3, b.h_img.ptr, None, b.cap, t.mem.stream) == E_ARG
    check_read(t.read(b), files)
    return 11
