"""Checks of the PNG writer (zmi_png_encode_dev, include/zmi355.h), shared by tests/test_png_write_craft.py (CPU, no library: the
judges against each other), tests/test_emu_png_write.py (CPU, the emulator build) and tests/test_gpu_png_write.py (the MI355X), the
last two through the C ABI on buffers a `mem` object owns (put / full / read / stream, as in tests/png_checks.py).

The judges, none of them the code under test:
  (a) choose(): the filter type of every row from five png_checks.filter_rows candidates, cost sum(v if v < 128 else 256 - v), the
      smallest type on ties; scanlines() = the rows filtered with those types (or with the one fixed type);
  (b) craft(): the whole expected file from struct.pack, its payload from the existing zmi_deflate_pieces_dev(ZMI_STREAM_INDEPENDENT,
      final_piece = 1) on the expected scanlines' pieces alone, Adler-32 and CRC-32 from zlib -- compared byte for byte at the levels
      of EXACT (at levels 1 and 3 the encoder's bytes depend on the launch: DESIGN.md section 19);
  (c) parse(): the file taken apart in Python -- signature, the three chunks and their CRC-32 --, zlib.decompress of the IDAT data must
      be the expected scanlines exactly (this judges the filter kernel at every level), png_checks.unfilter of them the pixels;
  (d) PIL, where it imports: Image.open(...).load() gives the pixels for depth 8 and for 16-bit gray;
  (e) the library's reader: zmi_png_headers_dev of the output is d_written, zmi_png_decode_dev returns the input pixels."""
import ctypes as C
import functools
import io
import struct
import types
import zlib

import numpy as np

import png_checks as P
from png_checks import E_ARG, Z_BUF_ERROR, NATIVE16, IMAGE, FORMATS, SHIFTS, CHANNELS, SIGNATURE, filter_rows, unfilter, paeth, chunk, pixels

ADAPTIVE = 5
GUARD, FILL, CANARY = 64, 0xC7, 0x77
EXACT = (0, 6, 9)

try:
    from PIL import Image
except ImportError:                                          # judge (d) is then left out
    Image = None


def bind(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    P.bind(L)
    L.zmi_png_filter_tile.restype = u32
    L.zmi_png_filter_tile.argtypes = []
    L.zmi_png_bound.restype = u64
    L.zmi_png_bound.argtypes = [u32, u64, u32, u32, i32]
    L.zmi_png_encode_dev.argtypes = [vp, vp, vp, vp, vp, u32, u64, u32, u32, u32, i32, i32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_deflate_pieces_stride.restype = u64
    L.zmi_deflate_pieces_stride.argtypes = [u32]
    L.zmi_deflate_pieces_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, u32, i32, vp, u64, vp, vp, vp, vp]
    return L


# ---- the images ------------------------------------------------------------------------------------------------------------------------------
class Img:
    """One image: `raw` its height * row_bytes bytes with big-endian samples (what the file says).  table / length: what the device
    table and the length table hold where that is not the image's own (the status checks)."""

    def __init__(self, width, height, colour=0, depth=8, seed=1, raw=None, table=None, length=None):
        self.width, self.height, self.colour, self.depth = width, height, colour, depth
        self.channels = CHANNELS[colour]
        self.row_bytes = (width * self.channels * depth + 7) // 8
        self.bpp = max(1, self.channels * depth // 8)
        n = height * self.row_bytes
        self.raw = pixels(n, seed) if raw is None else bytes(raw)
        assert len(self.raw) == n
        self.table, self.length = table, length
        self.bad = table is not None or length is not None

    def data(self, native16):
        return P.swap16(self.raw) if native16 and self.depth == 16 else self.raw

    @property
    def scan_bytes(self):
        return 0 if self.bad else (1 + self.row_bytes) * self.height

    def key(self):
        return (self.width, self.height, self.colour, self.depth, self.raw)


def cost(filtered):
    return sum(v if v < 128 else 256 - v for v in filtered)


def candidates(raw, height, row_bytes, bpp):
    """[t][r] = row r filtered with type t (without the filter byte)"""
    out = []
    for t in range(5):
        scan = filter_rows(raw, height, row_bytes, bpp, [t] * height)
        out.append([scan[r * (1 + row_bytes) + 1:(r + 1) * (1 + row_bytes)] for r in range(height)])
    return out


def choose(raw, height, row_bytes, bpp):
    """judge (a): the type of every row, and the costs [r][t] it was chosen from"""
    cand = candidates(raw, height, row_bytes, bpp)
    costs = [[cost(cand[t][r]) for t in range(5)] for r in range(height)]
    return [min(range(5), key=lambda t: (costs[r][t], t)) for r in range(height)], costs


@functools.lru_cache(maxsize=None)
def _scanlines(key, filt):
    width, height, colour, depth, raw = key
    ch = CHANNELS[colour]
    rb, bpp = (width * ch * depth + 7) // 8, max(1, ch * depth // 8)
    types_ = choose(raw, height, rb, bpp)[0] if filt == ADAPTIVE else [filt] * height
    return filter_rows(raw, height, rb, bpp, types_)


def scanlines(img, filt):
    return _scanlines(img.key(), filt)


def scanlines_none(img):
    """filter 0 without the byte loop, for images of megabytes"""
    a = np.frombuffer(img.raw, dtype=np.uint8).reshape(img.height, img.row_bytes)
    return np.concatenate([np.zeros((img.height, 1), dtype=np.uint8), a], axis=1).tobytes()


def zlib_header(level, strategy):
    """RFC 1950: CMF 0x78, FLEVEL as zlib derives it from level and strategy, FCHECK"""
    level = 6 if level == -1 else level
    fl = 0 if strategy >= 2 or level < 2 else (1 if level < 6 else (2 if level == 6 else 3))
    h = 0x78 << 8 | fl << 6
    h += 31 - h % 31
    return struct.pack(">H", h)


def craft(img, scan, payload, level, strategy):
    """judge (b): the file the header describes around a given deflate payload"""
    ihdr = struct.pack(">IIBBBBB", img.width, img.height, img.depth, img.colour, 0, 0, 0)
    idat = zlib_header(level, strategy) + payload + struct.pack(">I", zlib.adler32(scan))
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def parse(file):
    """judge (c): (width, height, depth, colour, the inflated IDAT data) of a file of exactly signature, IHDR, one IDAT, IEND"""
    assert file[:8] == SIGNATURE, file[:8]
    at, chunks = 8, []
    while at < len(file):
        ln, ctype = struct.unpack_from(">I4s", file, at)
        data = file[at + 8:at + 8 + ln]
        assert len(data) == ln and struct.unpack_from(">I", file, at + 8 + ln)[0] == zlib.crc32(ctype + data), (ctype, "CRC-32")
        chunks.append((ctype, data))
        at += 12 + ln
    assert at == len(file) and [c for c, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [c for c, _ in chunks]
    assert len(chunks[0][1]) == 13 and chunks[2][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (comp, filt, lace) == (0, 0, 0)
    d = zlib.decompressobj()
    scan = d.decompress(chunks[1][1])
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return w, h, depth, colour, scan


def pil_pixels(file):
    """judge (d): the pixels PIL reads, in the file's byte order; None where PIL's mode does not keep them (or PIL is missing)"""
    if Image is None:
        return None
    im = Image.open(io.BytesIO(file))
    im.load()
    if im.mode in ("L", "LA", "RGB", "RGBA"):
        return im.tobytes()
    if im.mode in ("I;16", "I;16B", "I;16L", "I;16N"):
        a = np.asarray(im).astype(">u2")
        return a.tobytes()
    return None


# ---- the target ---------------------------------------------------------------------------------------------------------------------------
class Res:
    def __init__(self, rc, off=None, length=None, status=None, written=None, out=None, cap=0, guard_ok=True):
        self.rc, self.off, self.len, self.status, self.written, self.out, self.cap, self.guard_ok = rc, off, length, status, written, out, cap, guard_ok

    def file(self, i):
        return self.out[self.off[i]:self.off[i] + self.len[i]]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.tile = int(self.L.zmi_png_filter_tile())
        self.reader = P.Target(L, ctx, mem)
        self._payloads = {}

    def lay_out(self, imgs, native16=True, shift=0, gap=3):
        """the pixels one image behind the other, `gap` bytes of 0xEE between them -> (handles of data, offsets, lengths, table)"""
        m, blob, offs = self.mem, bytearray(), []
        for k, im in enumerate(imgs):
            blob += b"\xEE" * (gap + k % 3 if gap else 0)
            offs.append(len(blob))
            blob += im.data(native16)
        tab = np.zeros(len(imgs) + 1, dtype=IMAGE)
        for k, im in enumerate(imgs):
            f = dict(width=im.width, height=im.height, depth=im.depth, colour=im.colour)
            f.update(im.table or {})
            for name, v in f.items():
                tab[k][name] = v
            tab[k]["status"] = 0x55                            # (only four fields are read)
            tab[k]["row_bytes"] = 0xDEAD
        lens = [len(im.raw) if im.length is None else im.length for im in imgs]
        return (m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift), m.put(np.array(offs + [0], dtype=np.uint64)),
                m.put(np.array(lens + [0], dtype=np.uint32)), m.put(tab))

    def encode(self, imgs, filt=ADAPTIVE, pb=4096, level=6, strategy=0, align=1, native16=True, shift=0, cap=None, scan_bytes=None,
               count=None, flags=None, written=True, null=None, handles=None):
        """one zmi_png_encode_dev call.  cap None: zmi_png_bound; handles: (data, offsets, lengths, table) that already stand on the
        device (the round trip)"""
        m, n, na = self.mem, len(imgs) if count is None else count, len(imgs)
        h_in, h_off, h_len, h_tab = handles or self.lay_out(imgs, native16, shift)
        if scan_bytes is None:
            scan_bytes = sum(im.scan_bytes for im in imgs)
        if cap is None:
            cap = int(self.L.zmi_png_bound(na, scan_bytes, pb, align if 1 <= align <= 4096 else 1, level))
        if flags is None:
            flags = NATIVE16 if native16 else 0
        out = m.full(GUARD + cap + GUARD, FILL)
        h_o, h_l, h_s = m.full((na + 2) * 8, CANARY), m.full((na + 1) * 4, CANARY), m.full((na + 1) * 4, CANARY)
        h_w = m.full((na + 1) * 48, CANARY)
        ptr = {"in": h_in.ptr, "off": h_off.ptr, "len": h_len.ptr, "tab": h_tab.ptr, "out": out.ptr + GUARD, "ooff": h_o.ptr, "olen": h_l.ptr,
               "st": h_s.ptr, "ctx": self.ctx}
        if null:
            ptr[null] = None
        rc = self.L.zmi_png_encode_dev(ptr["ctx"], ptr["in"], ptr["off"], ptr["len"], ptr["tab"], n, scan_bytes, flags, filt, pb, level, strategy,
                                       align, ptr["out"], cap, ptr["ooff"], ptr["olen"], h_w.ptr if written else None, ptr["st"], m.stream)
        if rc != 0:
            return Res(rc)
        off = [int(x) for x in m.read(h_o, np.uint64)]
        if n == 0:
            return Res(0, off[:1], [], [], None, b"", cap, off[1] == int.from_bytes(bytes([CANARY]) * 8, "little"))
        ln, st = [int(x) for x in m.read(h_l, np.uint32)], [int(x) for x in m.read(h_s, np.int32)]
        wr = m.read(h_w, IMAGE)
        word = int.from_bytes(bytes([CANARY]) * 8, "little")
        assert off[n + 1] == word and ln[n] == word & 0xFFFFFFFF and st[n] == word & 0xFFFFFFFF, "the call wrote behind its tables"
        assert wr[n:].tobytes() == bytes([CANARY]) * 48 and (written or wr.tobytes() == bytes([CANARY]) * 48 * (n + 1))
        buf = m.read(out, np.uint8)
        body = buf[GUARD:GUARD + cap]
        # nothing outside the files that are complete; a file that crosses out_cap may have left pieces in front of it
        touched = np.zeros(cap, dtype=bool)
        for i in range(n):
            if st[i] == 0:
                touched[off[i]:off[i] + ln[i]] = True
            elif st[i] == Z_BUF_ERROR:
                touched[min(off[i], cap):] = True
        ok = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all() and (body[~touched] == FILL).all())
        return Res(0, off[:n + 1], ln[:n], st[:n], wr[:n] if written else None, body.tobytes(), cap, ok)

    def payload(self, scan, pb, level, strategy):
        """judge (b)'s payload: the scanlines' pieces through zmi_deflate_pieces_dev alone, independent, the last one final"""
        key = (scan, pb, level, strategy)
        if key not in self._payloads:
            m = self.mem
            n = max(1, -(-len(scan) // pb))
            lens = [min(pb, len(scan) - i * pb) for i in range(n)]
            stride = int(self.L.zmi_deflate_pieces_stride(pb))
            inp, out = m.put(np.frombuffer(scan + b"\0" * 16, dtype=np.uint8)), m.full(n * stride, 0)
            od, ld = m.put(np.arange(n + 1, dtype=np.uint64) * pb), m.put(np.array(lens + [0], dtype=np.uint32))
            ol, st = m.full(4 * n, 0), m.full(4 * n, 0)
            rc = self.L.zmi_deflate_pieces_dev(self.ctx, inp.ptr, od.ptr, ld.ptr, n, pb, level, strategy, 0, 1, 1, out.ptr, stride, ol.ptr, None,
                                               st.ptr, m.stream)
            assert rc == 0, self.L.zmi_last_error()
            assert not m.read(st, np.int32).any()
            host, sizes = m.read(out, np.uint8), m.read(ol, np.uint32)
            self._payloads[key] = b"".join(host[i * stride:i * stride + int(sizes[i])].tobytes() for i in range(n))
        return self._payloads[key]

    def read_back(self, files, native16=True):
        """judge (e): -> (the records, the decoded regions) of the files through zmi_png_headers_dev and zmi_png_decode_dev"""
        b = self.reader.headers([types.SimpleNamespace(blob=f) for f in files], shift=3, gap=5)
        assert b.rc == 0
        r = self.reader.decode(b, flags=NATIVE16 if native16 else 0)
        assert r.rc == 0 and r.clean and r.status == [0] * len(files) and r.detail == [0] * len(files), (r.status, r.detail)
        return b.rec, [r.slot(j) for j in range(len(files))]


def expected_offsets(lengths, align):
    off, at = [], 0
    for ln in lengths:
        off.append(at)
        at += -(-ln // align) * align
    return off + [at]


def check(t, r, imgs, filt=ADAPTIVE, pb=4096, level=6, strategy=0, align=1, native16=True, scans=None, exact=None, pil=True):
    """every judge on a call that had room for all its files"""
    assert r.rc == 0 and r.guard_ok, (r.rc, r.guard_ok)
    n = len(imgs)
    assert r.status == [E_ARG if im.bad else 0 for im in imgs], r.status
    assert r.off == expected_offsets(r.len, align), (r.off[:8], r.len[:8])
    assert all((ln == 0) == im.bad for ln, im in zip(r.len, imgs))
    good = [i for i in range(n) if not imgs[i].bad]
    files = [r.file(i) for i in good]
    exact = level in EXACT if exact is None else exact
    for k, i in enumerate(good):
        im, f = imgs[i], files[k]
        scan = scans[i] if scans else scanlines(im, filt)
        w, h, depth, colour, got = parse(f)                                                   # (c)
        assert (w, h, depth, colour) == (im.width, im.height, im.depth, im.colour), (i, w, h, depth, colour)
        if got != scan:
            bad = next(q for q in range(min(len(got), len(scan))) if got[q] != scan[q]) if len(got) == len(scan) else -1
            st = 1 + im.row_bytes
            raise AssertionError("image %d (%dx%d colour %d depth %d): scanline byte %d (row %d, column %d) is %r, not %r; lengths %d / %d"
                                 % (i, im.width, im.height, im.colour, im.depth, bad, bad // st, bad % st - 1, got[bad] if bad >= 0 else None,
                                    scan[bad] if bad >= 0 else None, len(got), len(scan)))
        if scans is None:
            assert unfilter(got, h, im.row_bytes, im.bpp) == im.raw, i
        if exact:                                                                             # (b)
            want = craft(im, scan, t.payload(scan, pb, level, strategy), level, strategy)
            assert f == want, (i, len(f), len(want), next((q for q in range(min(len(f), len(want))) if f[q] != want[q]), None))
        if pil and (im.depth == 8 or (im.depth == 16 and im.colour == 0)):                    # (d)
            px = pil_pixels(f)
            assert px is None or px == im.raw, (i, "PIL")
    for i in range(n):                                                                        # d_written of a failed image
        if imgs[i].bad and r.written is not None:
            z = np.zeros(1, dtype=IMAGE)
            z[0]["status"] = E_ARG
            assert r.written[i].tobytes() == z.tobytes(), i
    if files:                                                                                 # (e)
        rec, regions = t.read_back(files, native16)
        for k, i in enumerate(good):
            assert regions[k] == imgs[i].data(native16), (i, "the reader's pixels")
            if r.written is not None:
                assert r.written[i].tobytes() == rec[k].tobytes(), (i, r.written[i], rec[k])
    return len(good)


def run(t, imgs, **kw):
    ekw = {k: v for k, v in kw.items() if k not in ("scans", "exact", "pil")}
    r = t.encode(imgs, **ekw)
    ckw = {k: v for k, v in kw.items() if k in ("filt", "pb", "level", "strategy", "align", "native16", "scans", "exact", "pil")}
    check(t, r, imgs, **ckw)
    return r


# ---- constructed inputs -----------------------------------------------------------------------------------------------------------------
def five_rows(width=32):
    """An 8-bit gray image built so that the chooser, and it alone, must pick FIVE_TYPES and has exact ties to break: row 0 a nonlinear
    ramp (None ties with Up, Sub with Paeth, as on every first row; Sub wins), row 1 the same ramp moved one pixel along the diagonal
    (Paeth alone predicts it exactly), row 2 a copy of the row above (Up), row 3 the mean of left and above (Average), row 4 a
    constant row of 0 (None ties with Sub at cost 0: None), row 5 a horizontal ramp (above a row of zeros Sub ties with Paeth: Sub),
    row 6 bytes of 0x80 between zeros (cost 128 either way; None).  tests/test_png_write_craft.py asserts all of that of the judge."""
    hfun = lambda k: 2 * k + k * k // 16                                                      # steps of 2 .. 8 that keep changing
    rows = [[hfun(i + 8) for i in range(width)]]
    rows.append([hfun(i + 7) for i in range(width)])                                          # x[r][i] = x[r - 1][i - 1]
    rows.append(list(rows[-1]))
    mean, left = [], 0
    for i in range(width):
        left = (left + rows[-1][i]) >> 1
        mean.append(left)
    rows.append(mean)
    rows.append([0] * width)
    rows.append([(7 * i + 3) & 0xFF for i in range(width)])
    rows.append([0x80 if i % 4 == 1 else 0 for i in range(width)])
    return Img(width, len(rows), 0, 8, raw=bytes(v for row in rows for v in row))


FIVE_TYPES = [1, 4, 2, 3, 0, 1, 0]
FIVE_TIES = {0: (1, 4), 2: (2, 4), 4: (0, 1), 5: (1, 4)}                # row: two types of exactly the same cost, one of them the winner


def stress(colour=2, depth=8, width=11, height=9, seed=5):
    """full-range noise with constant stretches: every outcome of Paeth and its ties, Average's carry, the first bpp bytes"""
    ch = CHANNELS[colour]
    rb = (width * ch * depth + 7) // 8
    r = np.random.RandomState(seed)
    a = r.randint(0, 256, (height, rb))
    a[:, rb // 2:rb // 2 + 6] = 255                                                           # a = b = c: the three-way tie; a + b = 510
    a[height // 2, :] = a[height // 2 - 1, :]                                                 # b = x
    a[2, 3:9] = np.arange(250, 256)[:len(a[2, 3:9])]                                                           # a + b >= 256 beside the noise
    return Img(width, height, colour, depth, raw=a.astype(np.uint8).tobytes())


def paeth_outcomes(img):
    """which of Paeth's branches the judge takes on the image: a set of 'a', 'b', 'c', 'tie'"""
    seen, rb, bpp, raw = set(), img.row_bytes, img.bpp, img.raw
    for r in range(1, img.height):
        for i in range(bpp, rb):
            a, b, c = raw[r * rb + i - bpp], raw[(r - 1) * rb + i], raw[(r - 1) * rb + i - bpp]
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            seen.add("a" if paeth(a, b, c) == a and pa < min(pb, pc) else ("b" if pb < min(pa, pc) else ("c" if pc < min(pa, pb) else "tie")))
            if a + b >= 256:
                seen.add("carry")
    return seen


def mixed(count, seed=7):
    """`count` tiny images of every writable format in turn, 1 .. 9 pixels a side"""
    fm = [f for f in FORMATS if f[0] != 3]
    return [Img(1 + (k * 5 + seed) % 9, 1 + (k * 3 + seed) % 7, fm[k % len(fm)][0], fm[k % len(fm)][1], seed=seed + k % 11) for k in range(count)]


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------------
def geometry(t, heights=(1, 2, 63, 64, 65, 129), widths=(1, 2, 63, 64, 65)):
    """every height against every width as RGB in one batch; row_bytes around the filter kernel's trip for pixels of 1, 3, 4 and 8
    bytes (the widths whose row_bytes are the nearest below tile, at or above it, the next one, above 2 * tile, and above 4 * tile, where whole trips lie inside the row); row_bytes 1"""
    imgs = [Img(w, h, 2, 8, seed=1 + (w + h) % 5) for h in heights for w in widths]
    run(t, imgs)
    done = len(imgs)
    T = t.tile
    for colour, depth, px in ((0, 8, 1), (2, 8, 3), (6, 8, 4), (6, 16, 8)):
        ws = [max(1, (T - 1) // px), -(-T // px), -(-T // px) + 1, -(-(2 * T + 1) // px), -(-(4 * T + 3) // px)]
        imgs = [Img(w, 3, colour, depth, seed=2 + px) for w in ws]
        run(t, imgs)
        done += len(imgs)
    imgs = [Img(1, h, 0, 8, seed=3) for h in (1, 2, 5)] + [Img(8, 3, 0, 1, seed=4), Img(3, 2, 0, 2, seed=4)]
    run(t, imgs)
    return done + len(imgs)


# ---- 2. formats -----------------------------------------------------------------------------------------------------------------------------
def formats(t, flags=(True, False)):
    """every depth / colour pair but the palette ones under both byte orders; packed depths at widths that leave padding bits"""
    done = 0
    for native16 in flags:
        imgs = []
        for colour, depth in FORMATS:
            if colour != 3:
                imgs += [Img(w, 5, colour, depth, seed=3 + depth) for w in ((5, 13) if depth < 8 else (7,))]
        run(t, imgs, native16=native16)
        done += len(imgs)
    return done


# ---- 3. filters -----------------------------------------------------------------------------------------------------------------------------
def filters(t):
    """each fixed type and the choice on the stress images (8-bit RGB, 16-bit RGBA, 4-bit gray) and on the constructed rows"""
    imgs = [stress(2, 8), stress(6, 16, 5, 7), stress(0, 4, 13, 6), five_rows()]
    for filt in (0, 1, 2, 3, 4, ADAPTIVE):
        run(t, imgs, filt=filt)
    r = t.encode([five_rows()])
    assert [parse(r.file(0))[4][k * 33] for k in range(7)] == FIVE_TYPES
    return 6 * len(imgs) + 1


def long_rows(t, flags=(True, False), filts=(0, 1, 2, 3, 4, ADAPTIVE)):
    """Rows long enough for trips that lie clear of both ends of the row, which run the filter kernel's variant without bounds tests and
    masks: one image per pixel distance 1, 2, 3, 4, 6, 8 (2 and 4 also as 16-bit samples) with row_bytes above 2 * tile + 16 + bpp and six
    rows, so that the row's misalignment in the scratch takes all four values; four 8-bit gray images whose row_bytes are 3 * tile + 8 - m
    for m 0 .. 3, so that for one misalignment a trip ends exactly where that variant's guard stops (x0 + tile + 8 == row_bytes).
    Every fixed type and the choice, under both byte orders, judged by the scanlines (c) and the other judges"""
    T = t.tile
    imgs = [Img(3 * T + 8 - m, 6, 0, 8, seed=2 + m) for m in range(4)]
    imgs += [Img(-(-(2 * T + 88) // px), 6, colour, depth, seed=3 + px + depth)
             for colour, depth, px in ((4, 8, 2), (0, 16, 2), (2, 8, 3), (6, 8, 4), (4, 16, 4), (2, 16, 6), (6, 16, 8))]
    assert all(im.row_bytes > 2 * T + 16 + im.bpp for im in imgs)
    for native16 in flags:
        for k, filt in enumerate(filts):
            run(t, imgs, filt=filt, native16=native16, pil=(k == 0))
    return len(flags) * len(filts) * len(imgs)


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------------
def batches(t, counts=(1, 3, 64, 65, 300), shifts=SHIFTS, aligns=(1, 16, 4096)):
    done = 0
    for count in counts:
        imgs = mixed(count)
        for k, shift in enumerate(shifts):
            run(t, imgs, shift=shift, align=aligns[k % len(aligns)], pil=(k == 0))
            done += 1
    return done


# ---- 5. pieces ------------------------------------------------------------------------------------------------------------------------------
def pieces(t, levels=(6, 9, 1)):
    """8 rows of 31 gray bytes, 256 scanline bytes: piece_bytes below a row, equal to 1 + row_bytes (every cut falls on a filter
    byte), one byte off that, the whole image, one byte less than it, and more than it; and piece_bytes 3: 86 pieces an image, more than
    the 64 a lane folds alone, so the Adler-32 and CRC-32 of the image come from the wave's fold"""
    im, done = Img(31, 8, 0, 8, seed=9), 0
    for level in levels:
        for pb in (7, 32, 31, 33, 256, 255, 257, 1 << 20, 3):
            run(t, [im, Img(5, 3, 2, 8), im], pb=pb, level=level)
            done += 1
    return done


def launch_group(t, limit, pb, max_len):
    """pieces a launch group holds under a scratch limit, as include/zmi355.h states it for zmi_zip_write_dev: the slot of
    zmi_deflate_pieces_stride plus the match scratch of 4 bytes a position and its sixteenth"""
    match = max(64, (max_len + 63) & ~63) * 4
    return limit // (int(t.L.zmi_deflate_pieces_stride(max_len)) + match + match // 16)


def across_groups(t, big=3 << 20, pb=1 << 20, front=10, behind=30, setenv=None, force=None):
    """one image of `big` bytes behind `front` tiny ones and in front of `behind` more, in launch groups the image lies across: under
    the smallest scratch limit there is (64 MiB), or, with `force`, in groups of that many pieces (ZMI_STREAM_GROUP); that it does lie
    across two groups is asserted.  Filter None, whose scanlines need no byte loop in the judge"""
    side = int((big // 3) ** 0.5)
    imgs = mixed(front) + [Img(side, side, 2, 8, seed=6)] + mixed(behind, seed=9)
    scans = [scanlines_none(im) for im in imgs]
    ref = run(t, imgs, filt=0, pb=pb, scans=scans, pil=False)
    first, last = front, front + -(-imgs[front].scan_bytes // pb) - 1                       # the image's places in the piece table
    group = force or launch_group(t, 64 << 20, pb, min(pb, sum(im.scan_bytes for im in imgs)))
    assert group >= 1 and first // group != last // group, (group, first, last)
    if force:
        setenv("ZMI_STREAM_GROUP", str(force))
    else:
        assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 64 << 20) == 0
    try:
        r = t.encode(imgs, filt=0, pb=pb)
    finally:
        if force:
            setenv("ZMI_STREAM_GROUP", None)
        assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 8 << 30) == 0
    assert (r.off, r.len, r.status, r.out) == (ref.off, ref.len, ref.status, ref.out) and r.written.tobytes() == ref.written.tobytes()
    return len(imgs)


# ---- 6. statuses ----------------------------------------------------------------------------------------------------------------------------
def arguments(t):
    """every ZMI_E_ARG the header names as a return value; n_images 0"""
    im, done = [Img(5, 4, 2, 8)], 0
    for kw in (dict(pb=0), dict(pb=(1 << 30) + 1), dict(level=10), dict(level=-2), dict(strategy=5), dict(strategy=-1), dict(align=0), dict(align=3),
               dict(align=8192), dict(flags=2), dict(flags=4), dict(filt=6), dict(filt=255), dict(count=1 << 31), dict(null="ooff"), dict(null="olen"),
               dict(null="st"), dict(null="tab"), dict(null="off"), dict(null="len"), dict(null="in"), dict(null="out"), dict(null="ctx"),
               dict(scan_bytes=(1 << 31) * 5, pb=1, cap=64)):
        assert t.encode(im, **kw).rc == E_ARG, kw
        done += 1
    r = t.encode([], cap=0)
    assert (r.rc, r.off, r.guard_ok) == (0, [0], True)
    r = t.encode(im, written=False)
    check(t, r, im)
    return done + 2


def statuses(t):
    """every per-image violation between good neighbours whose bytes do not change; scan_bytes too small"""
    good = [Img(9, 6, 2, 8, seed=2), Img(4, 7, 0, 16, seed=3), Img(6, 5, 6, 8, seed=4)]
    ref = run(t, good)
    bad = [Img(5, 4, 2, 8, table=dict(width=0)), Img(5, 4, 2, 8, table=dict(height=0)), Img(5, 4, 2, 8, table=dict(width=1 << 31)),
           Img(5, 4, 2, 8, table=dict(height=0xFFFFFFFF)), Img(5, 4, 2, 8, table=dict(depth=4)), Img(5, 4, 0, 8, table=dict(depth=3)),
           Img(5, 4, 0, 8, table=dict(colour=1)), Img(5, 4, 0, 8, table=dict(colour=7)), Img(5, 4, 3, 8), Img(5, 4, 3, 8, table=dict(depth=16)),
           Img(5, 4, 2, 8, length=59), Img(5, 4, 2, 8, length=61), Img(5, 4, 2, 8, length=0), Img(5, 4, 2, 8, table=dict(width=6)),
           Img(5, 4, 0, 8, table=dict(width=0x7F000000, height=1), length=0x7F000000), Img(5, 4, 0, 8, table=dict(width=0x7EFFFFFF, height=2))]
    for b in bad:
        b.bad = True
    for align in (1, 16):
        imgs = [good[0], bad[0], good[1]] + bad[1:] + [good[2]]
        r = run(t, imgs, align=align)
        assert [r.file(i) for i in (0, 2, len(imgs) - 1)] == [ref.file(i) for i in range(3)]
    r = run(t, bad)                                                                            # nothing but failures: no room is needed
    assert r.off == [0] * (len(bad) + 1)
    need = sum(im.scan_bytes for im in good)
    for sb in (need - 1, 0):
        r = t.encode(good, scan_bytes=sb, cap=ref.off[3])
        assert (r.rc, r.status, r.len, r.off, r.guard_ok) == (0, [E_ARG] * 3, [0] * 3, [0] * 4, True), (sb, r.status, r.off)
        assert r.out == bytes([FILL]) * r.cap
    r = t.encode(good, scan_bytes=need + 100000)                                               # a generous bound changes nothing
    assert [r.file(i) for i in range(3)] == [ref.file(i) for i in range(3)]
    return 2 + 1 + 2 + 1


def capacity(t):
    """out_cap at 0, one byte short of each file's end, exact: the files in front are complete, the one that crosses and those behind it
    are Z_BUF_ERROR with length 0, d_out_off is the plan of the lengths in all of them, nothing behind out_cap or in the gaps changes"""
    imgs, done = [Img(9, 6, 2, 8, seed=2), Img(40, 30, 0, 16, seed=3), Img(6, 5, 6, 8, seed=4)], 0
    for align in (1, 16, 4096):
        ref = run(t, imgs, align=align, pb=512)
        ends = [ref.off[i] + ref.len[i] for i in range(3)]
        for cap in [0] + [e - 1 for e in ends] + [ends[-1]]:
            r = t.encode(imgs, align=align, pb=512, cap=cap)
            fits = [e <= cap for e in ends]
            assert r.rc == 0 and r.guard_ok, (align, cap)
            assert r.off == ref.off and r.status == [0 if f else Z_BUF_ERROR for f in fits], (align, cap, r.off, r.status)
            assert r.len == [ln if f else 0 for ln, f in zip(ref.len, fits)]
            for i in range(3):
                if fits[i]:
                    assert r.file(i) == ref.file(i) and r.written[i].tobytes() == ref.written[i].tobytes()
                else:
                    z = np.zeros(1, dtype=IMAGE)
                    z[0]["status"] = Z_BUF_ERROR
                    assert r.written[i].tobytes() == z.tobytes()
            done += 1
    return done


# ---- 7. determinism -------------------------------------------------------------------------------------------------------------------------
def determinism(t, setenv, levels=(6, 1)):
    """one image alone, last of 300, at every input shift, under the smallest scratch limit (which is asserted to hold these 300 pieces
    in ONE group: the limit itself must not change a byte; across_groups is the case of several) and in forced groups of 1, 3 and 7:
    the same bytes"""
    im, done = Img(37, 29, 2, 8, seed=8), 0
    for level in levels:
        kw = dict(pb=1024, level=level)
        one = t.encode([im], **kw).file(0)
        parse(one)
        many = mixed(299) + [im]
        r = t.encode(many, **kw)
        assert r.status == [0] * 300 and r.file(299) == one
        for shift in SHIFTS[1:]:
            assert t.encode([im], shift=shift, align=16, **kw).file(0) == one
        assert launch_group(t, 64 << 20, 1024, 1024) >= 300 + sum(im.scan_bytes for im in many) // 1024
        assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 64 << 20) == 0
        try:
            r2 = t.encode(many, **kw)
        finally:
            assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 8 << 30) == 0
        assert r2.rc == 0 and (r2.off, r2.len, r2.out) == (r.off, r.len, r.out)
        try:
            for g in ("1", "3", "7"):
                setenv("ZMI_STREAM_GROUP", g)
                assert t.encode([im, im], **kw).file(1) == one
                done += 1
        finally:
            setenv("ZMI_STREAM_GROUP", None)
        done += 3
    return done


# ---- 8. the round trip across the two calls -------------------------------------------------------------------------------------------------
def round_trip(t, native16=True):
    """files of the crafter are read by zmi_png_headers_dev / zmi_png_decode_dev and written again from that table and that buffer as
    they stand on the device; the palette file and the broken one are ZMI_E_ARG there, the others decode to the same pixels"""
    pngs = [P.Png(9, 7, 2, 8, types=[0, 1, 2, 3, 4, 1, 2], seed=2), P.Png(5, 6, 0, 16, types=4, seed=3), P.Png(13, 4, 0, 1, types=3, seed=4),
            P.Png(6, 5, 3, 4, types=1, seed=5), P.Png(7, 3, 6, 16, types=2, split=(10, 7), seed=6), P.Png(4, 4, 4, 8, bad_crc=("IDAT",), seed=7),
            P.Png(70, 66, 2, 8, types=P.adaptive(66), seed=8)]
    m, rd, n = t.mem, t.reader, len(pngs)
    b = rd.headers(pngs, shift=1)
    flags = NATIVE16 if native16 else 0
    sizes = [p.height * p.row_bytes for p in pngs]
    cap = sum(-(-s // 16) * 16 for s in sizes)
    h_out, h_o, h_l = m.full(cap + 16, FILL), m.full((n + 1) * 8, 0), m.full(n * 4, 0)
    h_s, h_d = m.full(n * 4, 0), m.full(n * 4, 0)
    rc = t.L.zmi_png_decode_dev(t.ctx, b.h_in.ptr, b.h_off.ptr, b.h_len.ptr, b.h_img.ptr, n, None, n, flags, 16, h_out.ptr, cap, h_o.ptr, h_l.ptr,
                                h_s.ptr, h_d.ptr, m.stream)
    assert rc == 0
    imgs = [Img(p.width, p.height, p.colour, p.depth, raw=p.raw) for p in pngs]
    imgs[3].bad = imgs[5].bad = True                                                          # colour type 3; a length of 0 from the failed decode
    scan_bytes = sum((1 + p.row_bytes) * p.height for p in pngs)
    r = t.encode(imgs, handles=(h_out, h_o, h_l, b.h_img), scan_bytes=scan_bytes, native16=native16)
    check(t, r, imgs, native16=native16)
    return n


def engine_layer(e, torch):
    """the Engine calls: a list of tensors of mixed shapes and dtypes, save_png opened by PIL, the ValueErrors, png_encode of a PngBatch"""
    import pytest
    dev = e.device
    g = torch.Generator().manual_seed(3)
    ts = [torch.randint(0, 256, (7, 9, 3), dtype=torch.uint8, generator=g), torch.randint(0, 256, (5, 4), dtype=torch.uint8, generator=g),
          torch.randint(0, 65536, (6, 3, 4), dtype=torch.int32, generator=g).to(torch.uint16), torch.randint(0, 256, (3, 8, 1), dtype=torch.uint8, generator=g),
          torch.randint(-32768, 32768, (4, 5, 2), dtype=torch.int32, generator=g).to(torch.int16)]
    assert e.last_png_written is None
    out, off, ln, st = e.png_encode([x.to(dev) for x in ts])
    written = e.last_png_written
    assert st.tolist() == [0] * 5
    host, off, ln = out.cpu().numpy().tobytes(), off.tolist(), ln.tolist()
    colours = {1: 0, 2: 4, 3: 2, 4: 6}
    for k, x in enumerate(ts):
        w, h, depth, colour, scan = parse(host[off[k]:off[k] + ln[k]])
        c = 1 if x.dim() == 2 else x.shape[2]
        assert (w, h, depth, colour) == (x.shape[1], x.shape[0], 8 * x.element_size(), colours[c])
        a = x.numpy().view(np.uint16 if x.element_size() == 2 else np.uint8)
        raw = a.astype(">u2").tobytes() if x.element_size() == 2 else a.tobytes()
        assert unfilter(scan, h, len(raw) // h, max(1, c * x.element_size())) == raw, k
    blob = e.save_png(ts[0].to(dev), level=9)
    assert isinstance(blob, bytes) and parse(blob)[:4] == (9, 7, 8, 2)
    if Image is not None:
        assert pil_pixels(blob) == ts[0].numpy().tobytes()
    for wrong in ([ts[0]], [ts[0].to(dev).float()], [ts[0].to(dev)[None, None]], [torch.zeros((2, 2, 5), dtype=torch.uint8, device=dev)], []):
        with pytest.raises(ValueError):
            e.png_encode(wrong)
    with pytest.raises(ValueError):
        e.png_encode([ts[0].to(dev)], filter="best")
    # a PngBatch back into files: headers, decode, encode, and the reader again
    files = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
    batch = e.png_headers(files, torch.tensor(off[:5], dtype=torch.int64), torch.tensor(ln, dtype=torch.int64))
    data, doff, dlen, dst = e.png_decode(None, batch=batch)
    assert dst.tolist() == [0] * 5
    assert torch.equal(written, batch.images)                                       # the writer's table is the reader's
    scan_bytes = sum((1 + x.shape[1] * (1 if x.dim() == 2 else x.shape[2]) * x.element_size()) * x.shape[0] for x in ts)
    _, _, _, st3 = e.png_encode((data, doff[:5], dlen, batch), scan_bytes=scan_bytes - 1)     # the caller's bound is passed on
    assert st3.tolist() == [-103] * 5
    out2, off2, ln2, st2 = e.png_encode((data, doff[:5], dlen, batch), scan_bytes=scan_bytes)
    assert st2.tolist() == [0] * 5 and ln2.tolist() == ln and out2.cpu().numpy().tobytes()[:off[5]] == host[:off[5]] and off2.tolist() == off
    return 5
