"""Checks of the PNG reader (zmi_png_headers_dev / zmi_png_decode_dev, include/zmi355.h), shared by tests/test_emu_png.py (CPU, the
emulator build) and tests/test_gpu_png.py (the MI355X), both through the C ABI on buffers a `mem` object owns (put / full / read /
stream, as in tests/zip_checks.py).

The judges are two pieces of code in this file, neither of them the code under test: the crafter (struct.pack, zlib, forward filters
of its own; explicit filter type per row, an IDAT split list, placed faults) and `unfilter`, a byte-by-byte reference written from
section 9.2 of the PNG specification.  tests/test_png_craft.py pins both against PIL where PIL can be imported, and against each other
everywhere.  What a faulty zlib stream must report is judged by zlib.decompressobj."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR, Z_VERSION_ERROR, E_ARG = -3, -4, -5, -6, -103
(PE_SIGNATURE, PE_IHDR, PE_INTERLACE, PE_TRUNC, PE_CRITICAL, PE_ORDER, PE_BIG, PE_CRC, PE_DATA, PE_LENGTH, PE_FILTER, PE_OUT,
 PE_SCRATCH) = range(1, 14)
NATIVE16, NO_CRC = 1, 2
GUARD, FILL, CANARY = 64, 0xC7, 0x77
IMAGE = np.dtype([("width", "<u4"), ("height", "<u4"), ("depth", "u1"), ("colour", "u1"), ("channels", "u1"), ("bpp", "u1"),
                  ("row_bytes", "<u4"), ("idat_pos", "<u4"), ("n_idat", "<u4"), ("idat_bytes", "<u4"), ("plte_pos", "<u4"),
                  ("plte_len", "<u4"), ("trns_pos", "<u4"), ("trns_len", "<u4"), ("status", "<i4")])
assert IMAGE.itemsize == 48
SHIFTS = [0, 1, 3, 15]
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (4, 8), (4, 16), (2, 8), (2, 16), (6, 8), (6, 16), (3, 1), (3, 2), (3, 4), (3, 8)]


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_png_strip.restype = u32
    L.zmi_png_strip.argtypes = []
    L.zmi_png_headers_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.zmi_png_decode_dev.argtypes = [vp, vp, vp, vp, vp, u32, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_ctx_set_inflate_out_limit.argtypes = [vp, u64]
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    return L


# ---- the reference unfilter and the crafter's forward filters (section 9.2) ----------------------------------------------------------------
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def unfilter(scan, height, row_bytes, bpp):
    """the filtered scanlines -> the image's bytes; None where a filter byte is above 4"""
    out = bytearray(height * row_bytes)
    for r in range(height):
        t = scan[r * (1 + row_bytes)]
        if t > 4:
            return None
        f = scan[r * (1 + row_bytes) + 1:(r + 1) * (1 + row_bytes)]
        at, up = r * row_bytes, (r - 1) * row_bytes
        for i in range(row_bytes):
            a = out[at + i - bpp] if i >= bpp else 0
            b = out[up + i] if r > 0 else 0
            c = out[up + i - bpp] if r > 0 and i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[t]
            out[at + i] = (f[i] + pred) & 0xFF
    return bytes(out)


def filter_rows(raw, height, row_bytes, bpp, types):
    """the image's bytes -> filtered scanlines with the given type per row (a type above 4 is written as None under that byte)"""
    scan = bytearray()
    for r in range(height):
        t = types[r]
        row = raw[r * row_bytes:(r + 1) * row_bytes]
        up = raw[(r - 1) * row_bytes:r * row_bytes] if r > 0 else bytes(row_bytes)
        scan.append(t)
        for i in range(row_bytes):
            a = row[i - bpp] if i >= bpp else 0
            b = up[i]
            c = up[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[t] if t <= 4 else 0
            scan.append((row[i] - pred) & 0xFF)
    return bytes(scan)


def swap16(data):
    return np.frombuffer(data, dtype=">u2").astype("<u2").tobytes()


@functools.lru_cache(maxsize=None)
def pixels(n, seed=1):
    """n bytes: a smooth ramp with noise on top and runs of a constant, so that every filter gets something to do"""
    r = np.random.RandomState(seed)
    ramp = (np.arange(n) * (3 + seed % 5) // 7) & 0xFF
    noise = r.randint(0, 256, n) * (r.randint(0, 4, n) == 0)
    out = (ramp + noise) & 0xFF
    if n > 40:
        out[n // 3:n // 3 + 17] = 255
    return out.astype(np.uint8).tobytes()


def chunk(ctype, data, bad_crc=False, length=None):
    crc = zlib.crc32(ctype + data) ^ (0x00010000 if bad_crc else 0)
    return struct.pack(">I", len(data) if length is None else length) + ctype + data + struct.pack(">I", crc)


class Png:
    """One crafted file.  types: a filter type for every row (an int: for all rows); split: the lengths of the first IDAT chunks, the
    rest of the stream goes into one more; pre / mid / post: whole chunks in front of the first IDAT, behind the k-th IDAT (mid = (k,
    bytes)), and between the last IDAT and IEND.  Faults: bad_crc (a set of chunk types, or 'IDAT1' for the second IDAT), stream (the
    zlib stream itself), junk (bytes behind the stream inside IDAT), scan (the scanlines), ihdr (overrides of IHDR's fields), no_iend,
    trailing, signature.  `expect` = (status, detail) of a slot that decodes it, `want` its bytes (big-endian samples)."""

    def __init__(self, width, height, colour=0, depth=8, types=0, seed=1, level=6, split=(), raw=None, pre=b"", mid=None, post=b"",
                 bad_crc=(), stream=None, junk=b"", scan=None, ihdr=None, no_iend=False, trailing=b"", signature=SIGNATURE, plte=None,
                 interlace=0):
        self.width, self.height, self.colour, self.depth = width, height, colour, depth
        self.channels = CHANNELS[colour]
        self.row_bytes = (width * self.channels * depth + 7) // 8
        self.bpp = max(1, self.channels * depth // 8)
        self.types = [types] * height if isinstance(types, int) else list(types)
        assert len(self.types) == height
        n = height * self.row_bytes
        self.raw = pixels(n, seed) if raw is None else bytes(raw)
        assert len(self.raw) == n
        self.scan = filter_rows(self.raw, height, self.row_bytes, self.bpp, self.types) if scan is None else scan
        self.want = unfilter(self.scan, height, self.row_bytes, self.bpp) if len(self.scan) == (1 + self.row_bytes) * height else None
        if scan is None and max(self.types) <= 4:
            assert self.want == self.raw                                   # the crafter's filters against the reference unfilter
        self.stream = zlib.compress(self.scan, level) if stream is None else stream
        payload = self.stream + junk
        f = dict(width=width, height=height, depth=depth, colour=colour, comp=0, filt=0, lace=interlace)
        f.update(ihdr or {})
        out = bytearray(signature)
        out += chunk(b"IHDR", struct.pack(">IIBBBBB", f["width"], f["height"], f["depth"], f["colour"], f["comp"], f["filt"], f["lace"]),
                     "IHDR" in bad_crc)
        self.plte_pos = self.plte_len = 0
        if plte is None and colour == 3:
            plte = bytes((i * 37 + k * 11) & 0xFF for i in range(1 << depth) for k in range(3))
        if plte:
            self.plte_pos, self.plte_len = len(out) + 8, len(plte)
            out += chunk(b"PLTE", plte, "PLTE" in bad_crc)
        out += pre
        self.idat_pos = len(out)
        pieces, at = [], 0
        for ln in split:
            pieces.append(payload[at:at + ln])
            at += ln
        pieces.append(payload[at:])
        self.n_idat, self.idat_bytes = len(pieces), len(payload)
        for k, piece in enumerate(pieces):
            out += chunk(b"IDAT", piece, ("IDAT" in bad_crc and k == 0) or ("IDAT%d" % k) in bad_crc)
            if mid is not None and mid[0] == k:
                out += mid[1]
        out += post
        if not no_iend:
            out += chunk(b"IEND", b"", "IEND" in bad_crc)
        self.blob = bytes(out + trailing)
        self.flag = 0                                                      # the record's status
        self.expect = (0, 0)

    def flagged(self, code):
        self.flag = code
        self.expect = (Z_VERSION_ERROR if code in (PE_INTERLACE, PE_BIG) else Z_DATA_ERROR, code)
        return self

    def fails(self, detail, status=Z_DATA_ERROR):
        self.expect = (status, detail)
        return self

    def bytes_out(self, native16):
        return swap16(self.want) if native16 and self.depth == 16 else self.want


def judge_stream(payload, n):
    """what zlib says of a stream that must give exactly n bytes"""
    d = zlib.decompressobj()
    try:
        raw = d.decompress(payload, n + 1)
    except zlib.error:
        return Z_DATA_ERROR, PE_DATA
    if len(raw) != n or not d.eof:
        return Z_DATA_ERROR, PE_LENGTH
    return 0, 0


# ---- the target ---------------------------------------------------------------------------------------------------------------------------
class Batch:
    def __init__(self, rc, rec, h_in, h_off, h_len, h_img, n, pngs):
        self.rc, self.rec, self.h_in, self.h_off, self.h_len, self.h_img, self.n, self.pngs = rc, rec, h_in, h_off, h_len, h_img, n, pngs


class Read:
    def __init__(self, rc, off, length, status, detail, out, clean):
        self.rc, self.off, self.len, self.status, self.detail, self.out, self.clean = rc, off, length, status, detail, out, clean

    def slot(self, j):
        return self.out[self.off[j]:self.off[j] + self.len[j]]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.strip = int(self.L.zmi_png_strip())

    def headers(self, pngs, shift=0, gap=0, ctx="ctx"):
        """one zmi_png_headers_dev call on the files laid out one behind the other, `gap` bytes of 0xEE between them; a record of canary
        stands behind the table"""
        m, n = self.mem, len(pngs)
        blob, offs = bytearray(), []
        for k, p in enumerate(pngs):
            blob += b"\xEE" * (gap + (k * 5 % 7 if gap else 0))
            offs.append(len(blob))
            blob += p.blob
        h_in = m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift)
        h_off = m.put(np.array(offs + [0], dtype=np.uint64))
        h_len = m.put(np.array([len(p.blob) for p in pngs] + [0], dtype=np.uint32))
        h_img = m.full((n + 1) * 48, CANARY)
        rc = self.L.zmi_png_headers_dev(self.ctx if ctx == "ctx" else ctx, h_in.ptr, h_off.ptr, h_len.ptr, n, h_img.ptr, m.stream)
        if rc != 0:
            return Batch(rc, None, h_in, h_off, h_len, h_img, n, pngs)
        rec = m.read(h_img, IMAGE)
        assert bytes(rec[n:].tobytes()) == bytes([CANARY]) * 48, "the call wrote behind its table"
        return Batch(rc, rec[:n], h_in, h_off, h_len, h_img, n, pngs)

    def decode(self, b, sel=None, n_sel=None, flags=NATIVE16, align=1, cap=None, n_images=None, null=None, ctx="ctx"):
        """one zmi_png_decode_dev call on the batch; cap None: exactly the room the selection needs"""
        m = self.mem
        n_images = b.n if n_images is None else n_images
        if n_sel is None:
            n_sel = n_images if sel is None else len(sel)
        plan_off, plan_size = plan(b.rec[:n_images], sel, n_sel, align)
        need = plan_off[-1]
        if cap is None:
            cap = need
        h_sel = m.put(np.array(list(sel) + [0], dtype=np.uint32)) if sel is not None else None
        h_out = m.full(GUARD + cap + GUARD, FILL)
        h_o = m.full((n_sel + 2) * 8, CANARY)
        h_l = m.full((n_sel + 1) * 4, CANARY)
        h_s = m.full((n_sel + 1) * 4, CANARY)
        h_d = m.full((n_sel + 1) * 4, CANARY)
        args = dict(off=h_o.ptr, len=h_l.ptr, st=h_s.ptr, det=h_d.ptr)
        if null:
            args[null] = None
        rc = self.L.zmi_png_decode_dev(self.ctx if ctx == "ctx" else ctx, b.h_in.ptr, b.h_off.ptr, b.h_len.ptr, b.h_img.ptr, n_images,
                                       h_sel.ptr if h_sel else None, n_sel, flags, align, h_out.ptr + GUARD, cap, args["off"], args["len"],
                                       args["st"], args["det"], m.stream)
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


def plan(rec, sel, n_sel, align):
    """the offsets the contract gives: height * row_bytes of the readable slots in front, each rounded up to align; then the need"""
    off, sizes, at = [], [], 0
    align = align if 1 <= align <= 4096 and not align & (align - 1) else 1
    for j in range(n_sel):
        k = j if sel is None else sel[j]
        size = int(rec[k]["height"]) * int(rec[k]["row_bytes"]) if k < len(rec) and int(rec[k]["status"]) == 0 else 0
        off.append(at)
        sizes.append(size)
        at += -(-size // align) * align
    return off + [at], sizes


# ---- judges ---------------------------------------------------------------------------------------------------------------------------------
def check_records(b):
    """every record against what the crafter wrote"""
    assert b.rc == 0
    for k, (e, p) in enumerate(zip(b.rec, b.pngs)):
        assert int(e["status"]) == p.flag, (k, int(e["status"]), p.flag)
        if p.flag in (PE_SIGNATURE, PE_IHDR):
            continue
        got = tuple(int(e[f]) for f in ("width", "height", "depth", "colour", "channels", "bpp", "row_bytes"))
        assert got == (p.width, p.height, p.depth, p.colour, p.channels, p.bpp, p.row_bytes), (k, got)
        if p.flag == 0:
            got = tuple(int(e[f]) for f in ("idat_pos", "n_idat", "idat_bytes", "plte_pos", "plte_len"))
            assert got == (p.idat_pos, p.n_idat, p.idat_bytes, p.plte_pos, p.plte_len), (k, got)


def check_read(r, pngs, sel=None, flags=NATIVE16):
    """every slot's words and bytes, the offsets, the need, and nothing written elsewhere"""
    assert r.rc == 0 and r.clean, (r.rc, r.clean)
    assert r.off == r.plan_off, (r.off[:8], r.plan_off[:8])
    for j in range(len(r.status)):
        k = j if sel is None else sel[j]
        st, det = pngs[k].expect if k < len(pngs) else (E_ARG, 0)
        if det == PE_CRC and flags & NO_CRC:
            st, det = 0, 0
        assert (r.status[j], r.detail[j]) == (st, det), (j, k, r.status[j], r.detail[j], st, det)
        if st == 0:
            want = pngs[k].bytes_out(flags & NATIVE16)
            assert r.len[j] == len(want), (j, k, r.len[j], len(want))
            got = r.slot(j)
            if got != want:
                bad = next(i for i in range(len(want)) if got[i] != want[i])
                rb = pngs[k].row_bytes
                raise AssertionError("slot %d image %d: byte %d (row %d, column %d) is %d, not %d" % (j, k, bad, bad // rb, bad % rb, got[bad], want[bad]))
        else:
            assert r.len[j] == 0, (j, k)


def run(t, pngs, flags=NATIVE16, shift=0, align=1, gap=0, sel=None):
    """headers and decode of a batch, everything checked"""
    b = t.headers(pngs, shift=shift, gap=gap)
    check_records(b)
    r = t.decode(b, sel=sel, flags=flags, align=align)
    check_read(r, pngs, sel=sel, flags=flags)
    return b, r


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------------
def adaptive(height, seed=0):
    """a filter type per row that changes from row to row"""
    return [(r * 7 + seed + r // 5) % 5 for r in range(height)]


def geometry(t, heights=(1, 63, 64, 65, 129), widths=(1, 63, 64, 65)):
    """RGB and gray images of every height x width, adaptive filters and all-Paeth; then row_bytes around the strip; then row_bytes 1"""
    pngs = []
    for h in heights:
        for w in widths:
            pngs.append(Png(w, h, 2, 8, adaptive(h, w), seed=h + w))
            pngs.append(Png(w, h, 0, 8, 4, seed=h * w))
    S = t.strip
    for rb in (S - 1, S, S + 1, 2 * S + 3):
        pngs.append(Png(rb, 5, 0, 8, adaptive(5, rb), seed=rb))
        pngs.append(Png(rb, 3, 0, 8, 4, seed=rb + 1))
    for rb in (S - 2, S, S + 4):                                       # ... in pixels of four bytes, and of three (510 bytes a strip)
        pngs.append(Png(rb // 4, 4, 6, 8, [4, 3, 4, 1], seed=rb))
    for w in ((S // 3) - 1, S // 3, (S // 3) + 1):
        pngs.append(Png(w, 4, 2, 8, [1, 4, 3, 4], seed=w))
    for w in (1, 5, 8):                                                 # depth 1, at most 8 pixels: row_bytes 1
        pngs.append(Png(w, 7, 0, 1, adaptive(7, w), seed=w))
    run(t, pngs, align=16)
    return len(pngs)


# ---- 2. every format ------------------------------------------------------------------------------------------------------------------------
def formats(t, flag_sets=(NATIVE16, 0)):
    """every colour type / depth pair, so every bpp of 1, 2, 3, 4, 6 and 8, under both settings of NATIVE16"""
    pngs = [Png(13, 9, colour, depth, adaptive(9, colour + depth), seed=colour * 16 + depth) for colour, depth in FORMATS]
    assert sorted({p.bpp for p in pngs}) == [1, 2, 3, 4, 6, 8]
    for flags in flag_sets:
        run(t, pngs, flags=flags, align=16)
    return len(pngs) * len(flag_sets)


# ---- 3. filters -------------------------------------------------------------------------------------------------------------------------------
def filter_cases():
    pngs = []
    for ft in range(5):                                                 # each type on row 0, each type on every row
        pngs.append(Png(9, 3, 2, 8, [ft, 4, 3], seed=ft))
        pngs.append(Png(7, 6, 6, 8, ft, seed=10 + ft))
    for f0 in range(5):                                                 # all 25 ordered pairs on consecutive rows
        for f1 in range(5):
            pngs.append(Png(6, 3, 4, 8, [2, f0, f1], seed=f0 * 5 + f1))
    for at in (63, 64, 65):                                             # a chain start in front of, on and behind a band edge
        for ft in (0, 1):
            types = [4] * 130
            types[at] = ft
            pngs.append(Png(5, 130, 2, 8, types, seed=at + ft))
    pngs.append(Png(5, 200, 0, 8, [4] * 64 + [0] + [3] * 63 + [1] * 8 + [2] * 64, seed=3))   # starts on two band edges, then none
    pngs.append(Png(11, 70, 2, 8, 4, seed=5))                           # only Paeth: one chain
    pngs.append(Png(11, 70, 2, 8, 1, seed=6))                           # only Sub: every row could start one
    # Paeth ties: a == b == c; pa == pb < pc (a = b = c + d); pb == pc < pa (a = c + u, b = c - 2u)
    pngs.append(Png(6, 5, 0, 8, 4, raw=bytes([90]) * 30))
    pngs.append(Png(6, 5, 0, 8, 4, raw=bytes(50 if (r + i) % 2 else 40 for r in range(5) for i in range(6))))
    pngs.append(Png(4, 4, 0, 8, 4, raw=bytes(100 + 40 * i - 20 * r for r in range(4) for i in range(4))))
    pngs.append(Png(8, 4, 0, 8, 3, raw=bytes([255]) * 32))              # Avg with a = b = 255: the 9-bit sum
    pngs.append(Png(8, 3, 0, 8, 1, raw=bytes((i * 200) & 0xFF for i in range(24))))   # Sub wraps around
    return pngs


def filters(t):
    pngs = filter_cases()
    run(t, pngs, align=1)
    return len(pngs)


# ---- 4. the IDAT layout ---------------------------------------------------------------------------------------------------------------------
def idat_layout(t, many=300):
    pngs = []
    for level in (0, 1, 9):                                             # stored, fixed / dynamic blocks
        pngs.append(Png(40, 30, 2, 8, adaptive(30, level), seed=level, level=level))
        pngs.append(Png(40, 30, 2, 8, adaptive(30, level), seed=level, level=level, split=[100]))
    fixed = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    p = Png(20, 10, 0, 8, 2, seed=4)
    pngs.append(Png(20, 10, 0, 8, 2, seed=4, stream=fixed.compress(p.scan) + fixed.flush()))
    pngs.append(Png(30, 20, 6, 8, adaptive(20), seed=7, split=[1]))            # a first chunk of 1 byte: the zlib header is split
    pngs.append(Png(30, 20, 6, 8, adaptive(20), seed=8, split=[1, 0, 3]))
    pngs.append(Png(30, 20, 6, 8, adaptive(20), seed=9, split=[0, 50, 0, 0, 60]))    # zero-length chunks at the front and in the middle
    q = Png(30, 20, 6, 8, adaptive(20), seed=10)
    pngs.append(Png(30, 20, 6, 8, adaptive(20), seed=10, split=[70, len(q.stream) - 70]))   # ... and at the end
    pngs.append(Png(25, 40, 2, 8, adaptive(40), seed=11, level=0, split=[7] * (many - 1)))  # `many` chunks
    pngs.append(Png(30, 20, 2, 8, adaptive(20), seed=12, junk=b"junk behind the stream"))   # accepted
    pngs.append(Png(30, 20, 2, 8, adaptive(20), seed=13, junk=b"\0" * 40, split=[30, 30]))
    for p in pngs:
        if p.n_idat > 1:
            assert p.blob.count(b"IDAT") >= p.n_idat
    run(t, pngs, align=16, shift=3)
    return len(pngs)


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------------------
def mixed(n, seed=0):
    """n images of mixed shapes and formats, a few of several IDAT chunks"""
    pngs = []
    for i in range(n):
        colour, depth = FORMATS[(i + seed) % len(FORMATS)]
        w, h = 1 + (i * 7 + seed) % 23, 1 + (i * 5 + seed * 3) % 19
        if i == 1:
            w, h = 70, 67
        split = [9, 9] if i % 6 == 2 else ()
        pngs.append(Png(w, h, colour, depth, adaptive(h, i), seed=i + 1, level=(6, 1, 0, 9)[i % 4], split=split))
    return pngs


def batches(t, counts=(1, 3, 64, 65, 300), shifts=SHIFTS, aligns=(1, 16, 4096)):
    n = 0
    for count in counts:
        pngs = mixed(count)
        for k, shift in enumerate(shifts):
            run(t, pngs, shift=shift, align=aligns[k % len(aligns)], gap=shift)
            n += 1
    return n


# ---- 6. selection and room ------------------------------------------------------------------------------------------------------------------
def selection(t):
    pngs = mixed(7)
    pngs[4] = Png(9, 9, 0, 8, 0, interlace=1).flagged(PE_INTERLACE)
    b = t.headers(pngs)
    check_records(b)
    n = 0
    for sel in ([1, 3, 5], [6, 5, 4, 3, 2, 1, 0], [2, 2, 0, 2], [0, 7, 1, 4000000000, 2], []):
        for align in (1, 16):
            r = t.decode(b, sel=sel, align=align)
            if sel:
                check_read(r, pngs, sel=sel)
            else:
                assert r.rc == 0 and r.off == [0] and r.clean
            n += 1
    full = t.decode(b, align=16)
    check_read(full, pngs)
    need, end2 = full.need, full.off[1] + len(pngs[1].want)
    for cap in (need, need - 1, end2, 0):                               # (end2: the cap cuts behind the second image)
        r = t.decode(b, align=16, cap=cap)
        assert r.rc == 0 and r.clean and r.off == full.off and r.off[-1] == need
        for j, p in enumerate(pngs):
            if p.flag:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_VERSION_ERROR, PE_INTERLACE, 0)
            elif r.off[j] + len(p.want) <= cap:
                assert (r.status[j], r.detail[j], r.len[j]) == (0, 0, len(p.want)) and r.slot(j) == p.bytes_out(True), (cap, j)
            else:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_BUF_ERROR, PE_OUT, 0), (cap, j)
        n += 1
    return n


# ---- 7. every status code, among good neighbours ----------------------------------------------------------------------------------------------
def fault_cases():
    """-> [(name, Png)]"""
    def base(**kw):
        args = dict(colour=2, depth=8, types=adaptive(12, 3), seed=21)
        args.update(kw)
        return Png(10, 12, **args)

    good = base()
    n_scan = len(good.scan)
    row = 1 + good.row_bytes
    cases = []
    for ct in ("IHDR", "IDAT", "IEND"):
        cases.append(("crc " + ct, base(bad_crc={ct}).fails(PE_CRC)))
    cases.append(("crc PLTE", Png(10, 12, 3, 8, adaptive(12, 3), seed=21, bad_crc={"PLTE"}).fails(PE_CRC)))
    cases.append(("crc second IDAT", base(split=[20], bad_crc={"IDAT1"}).fails(PE_CRC)))
    cases.append(("crc ancillary", base(pre=chunk(b"tEXt", b"k\0v", bad_crc=True))))                         # ignored
    adler = good.stream[:-4] + struct.pack(">I", zlib.adler32(good.scan) ^ 1)
    assert judge_stream(adler, n_scan) == (Z_DATA_ERROR, PE_DATA)
    cases.append(("adler", base(stream=adler).fails(PE_DATA)))
    short = zlib.compress(good.scan[:-row])
    cases.append(("one row short", base(stream=short).fails(PE_LENGTH)))
    long_ = zlib.compress(good.scan + bytes(row))
    cases.append(("one row long", base(stream=long_).fails(PE_LENGTH)))
    cases.append(("one byte", base(stream=good.stream[:1]).fails(PE_LENGTH)))
    cases.append(("cut stream", base(stream=good.stream[:len(good.stream) // 2]).fails(PE_LENGTH)))
    bad = bytearray(good.stream)
    bad[len(bad) // 2] ^= 0x10
    cases.append(("corrupt", base(stream=bytes(bad)).fails(judge_stream(bytes(bad), n_scan)[1])))
    d = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, b"a preset dictionary")
    fdict = d.compress(good.scan) + d.flush()
    assert fdict[1] & 0x20
    cases.append(("fdict", base(stream=fdict).fails(PE_DATA)))
    scan5 = bytearray(good.scan)
    scan5[5 * row] = 5
    cases.append(("filter 5", base(scan=bytes(scan5)).fails(PE_FILTER)))
    cases.append(("adam7", base(interlace=1).flagged(PE_INTERLACE)))
    cases.append(("unknown critical", base(pre=chunk(b"CrIT", b"x")).flagged(PE_CRITICAL)))
    cases.append(("IDAT tEXt IDAT", base(split=[20], mid=(0, chunk(b"tEXt", b"k\0v"))).flagged(PE_ORDER)))
    leaves = base()
    at = leaves.idat_pos
    leaves.blob = leaves.blob[:at] + struct.pack(">I", len(leaves.blob)) + leaves.blob[at + 4:]
    cases.append(("chunk leaves the file", leaves.flagged(PE_TRUNC)))
    huge = base()
    huge.blob = huge.blob[:at] + struct.pack(">I", 0x80000000) + huge.blob[at + 4:]
    cases.append(("chunk length 2^31", huge.flagged(PE_TRUNC)))
    cases.append(("no IEND", base(no_iend=True).flagged(PE_TRUNC)))
    cases.append(("trailing bytes", base(trailing=b"behind IEND")))                                             # accepted
    apng = base(pre=chunk(b"acTL", struct.pack(">II", 2, 0)) + chunk(b"fcTL", bytes(26)),
                post=chunk(b"fcTL", bytes(26)) + chunk(b"fdAT", struct.pack(">I", 2) + good.stream))
    cases.append(("apng", apng))                                                                                # the default image decodes
    cases.append(("signature", base(signature=b"\x89PNG\r\n\x1a\r").flagged(PE_SIGNATURE)))
    cases.append(("no IHDR", Png(10, 12, 2, 8, 0, seed=21).flagged(PE_IHDR)))
    cases[-1][1].blob = SIGNATURE + chunk(b"gAMA", bytes(13)) + cases[-1][1].blob[33:]
    for name, ih in (("zero width", dict(width=0)), ("height 2^31", dict(height=1 << 31)), ("depth 3", dict(depth=3)),
                     ("rgb depth 4", dict(depth=4)), ("compression 1", dict(comp=1)), ("filter method 1", dict(filt=1)), ("interlace 2", dict(lace=2))):
        cases.append((name, base(ihdr=ih).flagged(PE_IHDR)))
    cases.append(("no IDAT", base().flagged(PE_ORDER)))
    p = cases[-1][1]
    p.blob = p.blob[:p.idat_pos] + chunk(b"IEND", b"")
    cases.append(("no PLTE", Png(10, 12, 3, 8, 0, seed=21, plte=b"").flagged(PE_ORDER)))
    cases.append(("PLTE behind IDAT", base(post=chunk(b"PLTE", bytes(6))).flagged(PE_ORDER)))
    cases.append(("PLTE length 7", Png(10, 12, 3, 8, 0, seed=21, plte=bytes(7)).flagged(PE_ORDER)))
    cases.append(("PLTE length 771", Png(10, 12, 3, 8, 0, seed=21, plte=bytes(771)).flagged(PE_ORDER)))
    big = base(ihdr=dict(width=0x7FFFFFFF, height=0x7FFFFFFF))
    big.width = big.height = 0x7FFFFFFF
    big.row_bytes = 0xFFFFFFFF
    cases.append(("big", big.flagged(PE_BIG)))
    big2 = base(ihdr=dict(width=20000, height=80000))
    big2.width, big2.height, big2.row_bytes = 20000, 80000, 60000
    cases.append(("scanlines of 4 GiB", big2.flagged(PE_BIG)))
    return cases


def statuses(t, flags=NATIVE16):
    """each fault as image 1 of three, the neighbours still decoding right; then all of them in one batch"""
    cases = fault_cases()
    left, right = Png(8, 70, 6, 16, adaptive(70), seed=31), Png(33, 5, 0, 4, adaptive(5), seed=32, split=[5])
    seen = set()
    for name, p in cases:
        try:
            run(t, [left, p, right], flags=flags, align=16)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        seen.add(p.expect[1])
    assert seen == set(range(0, PE_FILTER + 1)), sorted(seen)
    run(t, [left] + [p for _, p in cases] + [right], flags=flags)
    return len(cases)


def scratch(t):
    """the one status no placed fault in the file alone gives: an image of several IDAT chunks whose payload -- 80 KiB and more of junk
    behind its stream -- is longer than the gather buffer the call sizes from out_cap (2.125 x out_cap + 1 KiB a slot + 64 KiB).  It
    reports Z_MEM_ERROR / SCRATCH with length 0 and keeps its room; the several-IDAT image in front of it and the single-IDAT one behind
    it decode right; nothing is written outside the regions.  A several-IDAT image BEHIND it does not fit the buffer either."""
    left, right = Png(8, 70, 6, 16, adaptive(70), seed=31, split=[40, 40]), Png(33, 5, 0, 4, adaptive(5), seed=32)
    need = sum(len(p.want) for p in (left, right)) + 10 * 12 * 3 + 64
    fat = Png(10, 12, 2, 8, adaptive(12, 3), seed=21, split=[30], junk=bytes(range(256)) * (320 + need // 64)).fails(PE_SCRATCH, Z_MEM_ERROR)
    assert fat.idat_bytes > 2.125 * need + 3 * 1024 + 65536 + 4096
    run(t, [left, fat, right], align=16)
    run(t, [left, fat, right], align=1, shift=3, flags=NATIVE16 | NO_CRC)
    behind = Png(33, 5, 0, 4, adaptive(5), seed=32, split=[5]).fails(PE_SCRATCH, Z_MEM_ERROR)
    run(t, [left, fat, behind, right], align=16)
    return 3


def forged_record(t):
    """a record no headers call would write for its file -- the IDAT run it names leaves the file -- is ZMI_E_ARG in the slot, takes no
    room and nothing of it is read; the neighbours decode"""
    pngs = mixed(3)
    b = t.headers(pngs)
    n = 0
    for field, value in (("idat_bytes", len(pngs[1].blob) - int(b.rec[1]["idat_pos"]) - 23), ("idat_pos", len(pngs[1].blob) - 20), ("n_idat", 1 << 30)):
        rec = b.rec.copy()
        assert int(rec[1]["status"]) == 0
        rec[1][field] = value
        forged = Batch(0, rec.copy(), b.h_in, b.h_off, b.h_len, t.mem.put(rec), b.n, pngs)
        forged.rec[1]["status"] = -1                                      # (for the plan of this file: the slot takes no room)
        r = t.decode(forged)
        assert r.rc == 0 and r.clean and r.off == r.plan_off
        assert (r.status[1], r.detail[1], r.len[1]) == (E_ARG, 0, 0), (field, r.status[1], r.detail[1])
        for j in (0, 2):
            assert (r.status[j], r.detail[j]) == (0, 0) and r.slot(j) == pngs[j].bytes_out(True), (field, j)
        n += 1
    return n


def no_crc(t):
    """under NO_CRC an image with a flipped CRC is accepted, everything else stays"""
    pngs = [p for _, p in fault_cases()]
    assert sum(p.expect[1] == PE_CRC for p in pngs) == 5
    run(t, pngs, flags=NATIVE16 | NO_CRC)
    return len(pngs)


# ---- 8. determinism, 9. arguments -------------------------------------------------------------------------------------------------------------
def determinism(t):
    """the same words and bytes whatever the alignment of d_in, the number of images, the slot an image stands in and the context's
    scratch limits (the call sizes the decoder's bitmap itself, from out_cap: the context's inflate limit at its smallest, 1 MiB, and
    its scratch limit at its smallest, 64 MiB, change nothing)"""
    pngs = mixed(20)
    b0 = t.headers(pngs)
    ref = t.decode(b0)
    check_read(ref, pngs)
    assert t.L.zmi_ctx_set_inflate_out_limit(t.ctx, 1) == 0 and t.L.zmi_ctx_set_scratch_limit(t.ctx, 64 << 20) == 0
    try:
        r = t.decode(b0)
        assert (r.off, r.len, r.status, r.detail, r.out) == (ref.off, ref.len, ref.status, ref.detail, ref.out)
    finally:
        assert t.L.zmi_ctx_set_scratch_limit(t.ctx, 8 << 30) == 0
        t.L.zmi_ctx_set_inflate_out_limit(t.ctx, 0)                       # (the setter's floor is 1 MiB; the next inflate call sets its own)
    for shift in (1, 15):
        b = t.headers(pngs, shift=shift)
        assert b.rec["status"].tolist() == b0.rec["status"].tolist() and b.rec["idat_pos"].tolist() == b0.rec["idat_pos"].tolist()
        r = t.decode(b)
        assert (r.off, r.len, r.status, r.detail, r.out) == (ref.off, ref.len, ref.status, ref.detail, ref.out)
    for k in (0, 1, 19):
        one = t.decode(b0, sel=[k])
        assert (one.status, one.detail) == ([0], [0]) and one.slot(0) == pngs[k].bytes_out(True)
        alone = t.headers([pngs[k]])
        r = t.decode(alone)
        assert r.status == [0] and r.slot(0) == pngs[k].bytes_out(True)
    return 9


def arguments(t):
    pngs = mixed(3)
    b = t.headers(pngs)
    assert t.headers(pngs, ctx=None).rc == E_ARG
    assert t.decode(b, ctx=None).rc == E_ARG
    for align in (0, 3, 8192):
        assert t.decode(b, align=align).rc == E_ARG
    assert t.decode(b, flags=4).rc == E_ARG
    assert t.L.zmi_png_decode_dev(t.ctx, b.h_in.ptr, b.h_off.ptr, b.h_len.ptr, b.h_img.ptr, 3, None, 3, 0, 1, None, 0, None, None, None, None,
                                  t.mem.stream) == E_ARG
    assert t.decode(b, null="off").rc == E_ARG
    assert t.decode(b, null="st").rc == E_ARG
    assert t.L.zmi_png_headers_dev(t.ctx, b.h_in.ptr, None, b.h_len.ptr, 3, b.h_img.ptr, t.mem.stream) == E_ARG
    check_read(t.decode(b), pngs)
    return 10
