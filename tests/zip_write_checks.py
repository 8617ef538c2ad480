"""Checks of the ZIP writer (zmi_zip_bound / zmi_zip_write_dev, include/zmi355.h), shared by tests/test_emu_zip_write.py (CPU, the
emulator build) and tests/test_gpu_zip_write.py (the MI355X), both through the C ABI on buffers a `mem` object owns (put / full / read /
stream, as in tests/bgzf_checks.py).

Three judges, none of them the code under test:
  (a) Python's zipfile on every archive: testzip(), read() of every entry, and the fields the format section of the header fixes;
  (b) craft(): the whole expected archive from struct.pack, its payloads from the existing zmi_deflate_pieces_dev(ZMI_STREAM_INDEPENDENT,
      final_piece = 1) called on each entry's pieces alone with max_len = piece_bytes -- compared byte for byte at levels 0, 6 and 9;
  (c) the library's reader at base 0: zmi_zip_directory_dev gives the table and info the writer returned, zmi_zip_inflate_dev the input.
An archive that stands at file position `base` is opened behind PrefixFile, which presents `base` zero bytes in front of it."""
import ctypes as C
import io
import struct
import zipfile
import zlib

import numpy as np

import bgzf_checks as B

Z_BUF_ERROR, E_ARG = -5, -103
ENTRY_MAX = 0xF0000000
GUARD, FILL = 64, 0xA5
ROW = 48
DOS0, EXT0 = 0x00210000, 0x81A40000
LIMIT = 0xFFFFFFFF

SHIFTS = B.SHIFTS
CONFIGS = B.CONFIGS
KINDS = ["text", "mix", "zeros", "random"]
LENS_A = [0, 1, 4095, 4096, 4097, 3 * 4096, 3 * 4096 + 1]       # 1, 1, 1, 1, 2, 3 and 4 pieces of 4096
BASES = [0, LIMIT - 100, LIMIT - 31, 1 << 33]


def bind(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_deflate_pieces_stride.restype = u64
    L.zmi_deflate_pieces_stride.argtypes = [u32]
    L.zmi_deflate_pieces_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, u32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_zip_directory_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_zip_inflate_dev.argtypes = [vp, vp, u64, vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_zip_bound.restype = u64
    L.zmi_zip_bound.argtypes = [u32, u64, u64, u32, i32]
    L.zmi_zip_write_dev.argtypes = [vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, u32, i32, i32, u64, vp, u64, vp, vp, vp, vp, vp]
    return L


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def entries_of(kind, lens, seed=1):
    """one entry per length; "mix": text, zeros and random bytes in turn"""
    return [B.make(B.KINDS[i % 3] if kind == "mix" else kind, n, B.BLOCK_MAX, seed + i) for i, n in enumerate(lens)]


def names_of(count, seed=0):
    """distinct ASCII names of 1 .. 40 bytes"""
    return [("d%d/" % (i % 3) + "f%03d_" % (i + seed) + "x" * ((7 * i + seed) % 30) + ".bin").encode() for i in range(count)]


def date_time(dos):
    d, t = dos >> 16, dos & 0xFFFF
    return ((d >> 9) + 1980, (d >> 5) & 15, d & 31, t >> 11, (t >> 5) & 63, (t & 31) * 2)


# ---- judge (b): the crafter ---------------------------------------------------------------------------------------------------------------
class Crafted:
    def __init__(self, file, table, info, extras, locator):
        self.file, self.table, self.info, self.extras, self.locator = file, table, info, extras, locator


def craft(raws, names, payloads, method, base=0, dos=None, ext=None):
    """the archive the header describes, the zmi_zip_entry table and zmi_zip_info of it (positions: places in the archive), which
    entries carry the ZIP64 extra, and whether the ZIP64 record and locator are present"""
    n = len(raws)
    out, rows, cen, extras = bytearray(), [], [], []
    need = 20 if method else 10
    for i in range(n):
        raw, name, pay = raws[i], names[i], payloads[i]
        flags = 0x0800 if any(b >= 0x80 for b in name) else 0
        t = DOS0 if dos is None else dos[i]
        x = EXT0 if ext is None else ext[i]
        crc = zlib.crc32(raw)
        lho = len(out)
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, need, flags, method, t & 0xFFFF, t >> 16, crc, len(pay), len(raw), len(name), 0)
        out += name + pay
        a = base + lho
        sat = a >= LIMIT
        cneed = 45 if sat else need
        cen.append(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 0x0300 | cneed, cneed, flags, method, t & 0xFFFF, t >> 16, crc, len(pay),
                               len(raw), len(name), 12 if sat else 0, 0, 0, 0, x, LIMIT if sat else a)
                   + name + (struct.pack("<HHQ", 1, 8, a) if sat else b""))
        extras.append(sat)
        rows.append([lho + 30 + len(name), 0, len(pay), len(raw), crc, t, x, method, flags, len(name), 0, 0])
    cd = len(out)
    at = cd
    for i in range(n):
        rows[i][1] = at + 46
        at += len(cen[i])
    out += b"".join(cen)
    cd_size, cd_off = at - cd, base + cd
    z64 = n >= 0xFFFF or cd_size >= LIMIT or cd_off >= LIMIT
    if z64:
        rec = base + len(out)
        out += struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 0x032D, 45, 0, 0, n, n, cd_size, cd_off)
        out += struct.pack("<IIQI", 0x07064B50, 0, rec, 1)
    out += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(cd_size, LIMIT), min(cd_off, LIMIT), 0)
    table = b"".join(struct.pack("<QQIIIIIHHHHi", *r) for r in rows)
    info = struct.pack("<QQQQQii", n, n, cd, cd_size, 0, 0, 0)
    return Crafted(bytes(out), table, info, extras, z64)


# ---- the file object of an archive that stands at position `base` ----------------------------------------------------------------------------
class PrefixFile(io.RawIOBase):
    """`base` zero bytes, then `data`: what io.BytesIO(bytes(base) + data) is, without the bytes"""

    def __init__(self, data, base):
        super().__init__()
        self.data, self.base, self.pos = bytes(data), int(base), 0

    def seekable(self):
        return True

    def readable(self):
        return True

    def tell(self):
        return self.pos

    def seek(self, off, whence=0):
        p = off if whence == 0 else (self.pos + off if whence == 1 else self.base + len(self.data) + off)
        if p < 0:
            raise ValueError("negative seek position")
        self.pos = p
        return p

    def read(self, n=-1):
        end = self.base + len(self.data)
        if n is None or n < 0:
            n = max(0, end - self.pos)
        lo, hi = self.pos, min(self.pos + n, end)
        if hi <= lo:
            return b""
        zeros = max(0, min(hi, self.base) - lo)
        assert zeros <= 1 << 24, "a reader that walks the prefix"
        got = bytes(zeros) + (self.data[max(lo, self.base) - self.base:hi - self.base] if hi > self.base else b"")
        self.pos = hi
        return got


# ---- judge (a): zipfile -------------------------------------------------------------------------------------------------------------------
def check_zipfile(file, raws, names, method, base=0, dos=None, ext=None):
    """every entry read and compared, every field the format fixes; -> [(header offset, compressed size)]"""
    with zipfile.ZipFile(PrefixFile(file, base) if base else io.BytesIO(file)) as zf:
        infos = zf.infolist()
        assert len(infos) == len(raws), (len(infos), len(raws))
        assert zf.testzip() is None
        assert zf.comment == b""
        at, res = base, []
        for i, zi in enumerate(infos):
            name = names[i]
            utf = any(b >= 0x80 for b in name)
            assert zi.orig_filename == name.decode("utf-8" if utf else "cp437"), i
            assert zi.flag_bits == (0x0800 if utf else 0), (i, zi.flag_bits)
            assert zi.compress_type == method and zi.header_offset == at, (i, zi.compress_type, zi.header_offset, at)
            assert zi.date_time == date_time(DOS0 if dos is None else dos[i]), (i, zi.date_time)
            assert zi.external_attr == (EXT0 if ext is None else ext[i]), (i, zi.external_attr)
            assert zi.CRC == zlib.crc32(raws[i]) and zi.file_size == len(raws[i]), i
            assert zi.comment == b"" and zi.create_system == 3 and zi.internal_attr == 0, i
            if method == 0:
                assert zi.compress_size == len(raws[i]), i
            with zf.open(zi) as f:
                assert f.read() == raws[i], i
            res.append((zi.header_offset, zi.compress_size))
            at += 30 + len(name) + zi.compress_size                  # dense: the next header follows the payload
        assert zf.start_dir == at, (zf.start_dir, at)
    return res


def end_structure(file, base, n):
    """-> is the ZIP64 record + locator present; the end structure is checked against the rest of the file either way"""
    assert file[-22:-18] == b"PK\x05\x06" and file[-2:] == b"\0\0"
    loc = file[-42:-38] == b"PK\x06\x07"
    if loc:
        _, disk, rec, disks = struct.unpack("<IIQI", file[-42:-22])
        assert (disk, disks) == (0, 1) and rec == base + len(file) - 98 and file[-98:-94] == b"PK\x06\x06", (rec, base, len(file))
        assert struct.unpack("<QQ", file[-74:-58]) == (n, n)
    return loc


class Res:
    def __init__(self, rc, status=0, total=0, buf=b"", guard_ok=True, table=None, info=None):
        self.rc, self.status, self.total, self.buf, self.guard_ok, self.table, self.info = rc, status, total, buf, guard_ok, table, info

    @property
    def file(self):
        return self.buf[:self.total]

    def __repr__(self):
        return "Res(rc=%d status=%d total=%d guard_ok=%s)" % (self.rc, self.status, self.total, self.guard_ok)


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self._payloads, self._sizes = {}, {}

    def _bytes(self, b, shift=0):
        return self.mem.put(np.frombuffer(bytes(b) + b"\0" * 16, dtype=np.uint8), shift)

    def write(self, raws, names, pb=4096, level=6, strategy=0, base=0, shift=0, name_shift=1, dos=None, ext=None, cap=None, in_bytes=None,
              scattered=False, table=True, info=True, null=None, lens=None, count=None):
        """one zmi_zip_write_dev call.  scattered: the entries stand in reverse order with gaps of 3 bytes (any layout); lens: the
        length table the device sees, where it is not the entries' own; count: the n_entries the call is given, where it is not the
        number of entries (a count the host refuses before it reads a table)"""
        m, n = self.mem, len(raws)
        offs, blob = [0] * n, bytearray()
        for i in (reversed(range(n)) if scattered else range(n)):
            offs[i] = len(blob)
            blob += raws[i] + (b"\xEE" * 3 if scattered else b"")
        noff = [0]
        for nm in names:
            noff.append(noff[-1] + len(nm))
        if in_bytes is None:
            in_bytes = len(blob)
        if cap is None:
            cap = int(self.L.zmi_zip_bound(n, noff[-1], in_bytes, pb, level))
        inp, nmb, out = self._bytes(bytes(blob), shift), self._bytes(b"".join(names), name_shift), m.full(cap + GUARD, FILL)
        od = m.put(np.array(offs + [0], dtype=np.uint64))
        ld = m.put(np.array((lens if lens is not None else [len(r) for r in raws]) + [0], dtype=np.uint32))
        nd = m.put(np.array(noff, dtype=np.uint64))
        td = m.put(np.array(list(dos) + [0], dtype=np.uint32)) if dos is not None else None
        xd = m.put(np.array(list(ext) + [0], dtype=np.uint32)) if ext is not None else None
        olen, st = m.full(8, 0x77), m.full(4, 0x77)
        tab, inf = m.full((n + 1) * ROW, 0x77), m.full(ROW + 16, 0x77)
        ptr = {"ctx": self.ctx, "in": inp.ptr, "off": od.ptr, "len": ld.ptr, "names": nmb.ptr, "noff": nd.ptr, "out": out.ptr,
               "olen": olen.ptr, "st": st.ptr}
        if null:
            ptr[null] = None
        rc = self.L.zmi_zip_write_dev(ptr["ctx"], ptr["in"], ptr["off"], ptr["len"], n if count is None else count, in_bytes, ptr["names"], ptr["noff"],
                                      td.ptr if td else None, xd.ptr if xd else None, pb, level, strategy, base, ptr["out"], cap,
                                      ptr["olen"], tab.ptr if table else None, inf.ptr if info else None, ptr["st"], m.stream)
        if rc != 0:
            return Res(rc)
        host, t, f = m.read(out, np.uint8), m.read(tab, np.uint8).tobytes(), m.read(inf, np.uint8).tobytes()
        assert t[n * ROW:] == b"\x77" * ROW and f[ROW:] == b"\x77" * 16          # nothing behind the rows the call owns
        assert table or t == b"\x77" * len(t)
        assert info or f == b"\x77" * len(f)
        return Res(0, int(m.read(st, np.int32)[0]), int(m.read(olen, np.uint64)[0]), host[:cap].tobytes(), bool((host[cap:] == FILL).all()),
                   t[:n * ROW] if table else None, f[:ROW] if info else None)

    def payload(self, raw, pb, level, strategy):
        """judge (b)'s payload: the entry's pieces through zmi_deflate_pieces_dev alone, independent, the last one final"""
        if level == 0:
            return raw
        key = (raw, pb, level, strategy)
        if key not in self._payloads:
            m = self.mem
            n = max(1, -(-len(raw) // pb))
            lens = [min(pb, len(raw) - i * pb) for i in range(n)]
            stride = int(self.L.zmi_deflate_pieces_stride(pb))
            inp, out = self._bytes(raw), m.full(n * stride, 0)
            od, ld = m.put(np.arange(n + 1, dtype=np.uint64) * pb), m.put(np.array(lens + [0], dtype=np.uint32))
            ol, st = m.full(4 * n, 0), m.full(4 * n, 0)
            rc = self.L.zmi_deflate_pieces_dev(self.ctx, inp.ptr, od.ptr, ld.ptr, n, pb, level, strategy, 0, 1, 1, out.ptr, stride, ol.ptr, None,
                                               st.ptr, m.stream)
            assert rc == 0, self.L.zmi_last_error()
            assert not m.read(st, np.int32).any()
            host, sizes = m.read(out, np.uint8), m.read(ol, np.uint32)
            self._payloads[key] = b"".join(host[i * stride:i * stride + int(sizes[i])].tobytes() for i in range(n))
            self._sizes[key] = [int(x) for x in sizes[:n]]
        return self._payloads[key]

    def piece_sizes(self, raw, pb, level, strategy):
        """the bytes every piece of the entry takes in the archive"""
        if level == 0:
            return [min(pb, len(raw) - at) for at in range(0, max(1, len(raw)), pb)]
        self.payload(raw, pb, level, strategy)
        return self._sizes[(raw, pb, level, strategy)]

    def craft(self, raws, names, pb, level, strategy, **kw):
        return craft(raws, names, [self.payload(r, pb, level, strategy) for r in raws], 8 if level else 0, **kw)

    def read_back(self, file, n):
        """judge (c): -> (table, info, entries) from zmi_zip_directory_dev and zmi_zip_inflate_dev on the archive"""
        m = self.mem
        inp = self._bytes(file, 3)
        tab, inf = m.full(max(1, n) * ROW, 0), m.full(ROW, 0)
        rc = self.L.zmi_zip_directory_dev(self.ctx, inp.ptr, len(file), tab.ptr, n, inf.ptr, m.stream)
        assert rc == 0, self.L.zmi_last_error()
        t, f = m.read(tab, np.uint8).tobytes()[:n * ROW], m.read(inf, np.uint8).tobytes()
        assert struct.unpack("<QQQQQii", f)[0] == n
        total = sum(struct.unpack_from("<I", t, i * ROW + 20)[0] for i in range(n))
        out, ooff = m.full(total + 16, 0), m.full(8 * (n + 1), 0)
        olen, st, det = m.full(4 * max(1, n), 0), m.full(4 * max(1, n), 0x11), m.full(4 * max(1, n), 0x11)
        rc = self.L.zmi_zip_inflate_dev(self.ctx, inp.ptr, len(file), tab.ptr, n, None, n, 1, out.ptr, total, ooff.ptr, olen.ptr, st.ptr,
                                        det.ptr, m.stream)
        assert rc == 0, self.L.zmi_last_error()
        assert not m.read(st, np.int32)[:n].any() and not m.read(det, np.int32)[:n].any()
        host, off, ln = m.read(out, np.uint8), m.read(ooff, np.uint64), m.read(olen, np.uint32)
        assert int(off[n]) == total
        return t, f, [host[int(off[i]):int(off[i]) + int(ln[i])].tobytes() for i in range(n)]


def check_archive(target, res, raws, names, pb, level, strategy, base=0, dos=None, ext=None, exact=None, reader=True):
    """the three judges on one result; -> the crafted archive (None where the level is not byte-stable)"""
    assert res.rc == 0 and res.status == 0 and res.guard_ok, res
    method = 8 if level else 0
    got = check_zipfile(res.file, raws, names, method, base, dos, ext)
    if method == 8:
        for (_, csize), raw in zip(got, raws):
            assert csize >= 2 and (raw or csize == 2)
    want = None
    if exact if exact is not None else B.reproducible(level, strategy):
        want = target.craft(raws, names, pb, level, strategy, base=base, dos=dos, ext=ext)
        assert res.total == len(want.file) and res.file == want.file, (res, len(want.file))
        assert res.table == want.table and res.info == want.info
    if base == 0 and reader:
        t, f, back = target.read_back(res.file, len(raws))
        assert t == res.table and f == res.info
        assert back == list(raws)
    return want


# ---- 1. sizes and pieces -------------------------------------------------------------------------------------------------------------------
def shapes(target, configs=CONFIGS, kinds=KINDS, shifts=SHIFTS):
    done = 0
    names = names_of(len(LENS_A))
    for level, strategy in configs:
        for kind in kinds:
            raws = entries_of(kind, LENS_A)
            for shift in shifts:
                r = target.write(raws, names, 4096, level, strategy, shift=shift)
                check_archive(target, r, raws, names, 4096, level, strategy)
                done += 1
    return done


def small_pieces(target, configs=CONFIGS):
    """piece_bytes 1 with lengths 0 .. 3, and piece_bytes 1 << 20 with lengths 70 000 and 0"""
    done = 0
    for level, strategy in configs:
        raws = [B.make("text", n, seed=7)[:n] for n in range(4)]
        names = names_of(4)
        check_archive(target, target.write(raws, names, 1, level, strategy), raws, names, 1, level, strategy)
        raws = [B.make("mix", 70000, 30000), b""]
        names = names_of(2)
        check_archive(target, target.write(raws, names, 1 << 20, level, strategy, shift=3), raws, names, 1 << 20, level, strategy)
        done += 2
    return done


def many_pieces(target, levels=(6, 0)):
    """an entry of 71 pieces between two small ones: its CRC-32 is folded by the whole wave, the others' by one thread each"""
    raws = [B.make("text", 100, seed=3), B.make("mix", 64 * 70 + 5, 1500), b"z"]
    names = names_of(3)
    for level in levels:
        check_archive(target, target.write(raws, names, 64, level, shift=1), raws, names, 64, level, 0)
    return len(levels)


def random_expands(target):
    """random bytes at method 8 are longer than they were (no fallback to method 0, as zipfile), and the bound still holds"""
    raws = entries_of("random", [4096, 12289, 100])
    names = names_of(3)
    r = target.write(raws, names, 4096, 6, 0)
    check_archive(target, r, raws, names, 4096, 6, 0)
    sizes = [struct.unpack_from("<II", r.table, i * ROW + 16) for i in range(3)]
    assert all(c > u for c, u in sizes), sizes
    assert r.total <= int(target.L.zmi_zip_bound(3, sum(map(len, names)), sum(map(len, raws)), 4096, 6))
    return 1


# ---- 2. names and tables -------------------------------------------------------------------------------------------------------------------
def name_shapes(target, level=6):
    lens = [0, 1, 15, 16, 17, 255, 65535]
    names = [bytes(97 + (i + k) % 26 for k in range(n)) for i, n in enumerate(lens)]
    names += ["données/été 中.txt".encode("utf-8"), b"same/name", b"same/name"]
    raws = entries_of("text", [100 + 37 * i for i in range(len(names))])
    done = 0
    for name_shift in (1, 0):
        r = target.write(raws, names, 4096, level, name_shift=name_shift)
        check_archive(target, r, raws, names, 4096, level, 0)
        flags = [struct.unpack_from("<H", r.table, i * ROW + 38)[0] for i in range(len(names))]
        assert flags == [0] * 7 + [0x0800, 0, 0], flags
        done += 1
    long = bytes(65 + k % 26 for k in range(65536))
    r = target.write(raws[:3], [b"a", long, b"b"], 4096, level)
    assert (r.rc, r.status) == (0, E_ARG) and r.guard_ok, r
    r.status = 0
    check_archive(target, r, raws[:3], [b"a", long[:65535], b"b"], 4096, level, 0)        # cut to its first 65 535 bytes
    return done + 1


def tables(target, level=6):
    raws = entries_of("text", [300, 0, 5000])
    names = names_of(3)
    dos = [(2024 - 1980) << 25 | 2 << 21 | 29 << 16 | 23 << 11 | 59 << 5 | 29, DOS0, (2107 - 1980) << 25 | 12 << 21 | 31 << 16]
    ext = [0o100755 << 16, 0o40755 << 16 | 0x10, 0x81A40001]
    ref = None
    for d, x in ((dos, ext), (None, ext), (dos, None), (None, None)):
        r = target.write(raws, names, 4096, level, dos=d, ext=x)
        check_archive(target, r, raws, names, 4096, level, 0, dos=d, ext=x)
        ref = ref or r
    assert ref.file != r.file
    return 4


# ---- 3. grouping ---------------------------------------------------------------------------------------------------------------------------
def grouping(target, setenv, levels=(6, 0)):
    """launch groups of 3 and 7 pieces against one group: entries lie across group edges, the archives are equal"""
    names, done = names_of(len(LENS_A)), 0
    for level in levels:
        raws = entries_of("mix", LENS_A)
        one = target.write(raws, names, 4096, level)
        check_archive(target, one, raws, names, 4096, level, 0)
        try:
            for g in ("3", "7"):
                setenv("ZMI_STREAM_GROUP", g)
                r = target.write(raws, names, 4096, level)
                assert (r.rc, r.status, r.total, r.guard_ok) == (0, 0, one.total, True), (g, r)
                assert r.file == one.file and r.table == one.table and r.info == one.info, g
                done += 1
        finally:
            setenv("ZMI_STREAM_GROUP", None)
    return done


# ---- 4. ZIP64 ------------------------------------------------------------------------------------------------------------------------------
def zip64_base(target, levels=(6, 0), bases=BASES):
    """the archive of the first shape at file positions around 0xFFFFFFFF: which entries carry the extra, whether the locator is there"""
    names, done = names_of(len(LENS_A)), 0
    for level in levels:
        raws = entries_of("text", LENS_A)
        for base in bases:
            r = target.write(raws, names, 4096, level, base=base)
            want = check_archive(target, r, raws, names, 4096, level, 0, base=base, exact=True)
            heads = [struct.unpack_from("<Q", r.table, i * ROW)[0] - 30 - len(names[i]) for i in range(len(raws))]
            extras = [base + h >= LIMIT for h in heads]
            assert want.extras == extras
            if base == 0:
                assert not any(extras) and not end_structure(r.file, base, len(raws))
            elif base == LIMIT - 100:
                assert not extras[0] and extras[-1] and end_structure(r.file, base, len(raws))     # a later header crosses the limit
            elif base == LIMIT - 31:
                assert extras == [False] + [True] * 6 and end_structure(r.file, base, len(raws))   # the second header is the first
            else:
                assert all(extras) and end_structure(r.file, base, len(raws))
            # the extra is where the crafter put it: 12 more bytes in exactly those central records
            cd = struct.unpack_from("<Q", r.info, 16)[0]
            cd_size = struct.unpack_from("<Q", r.info, 24)[0]
            assert cd_size == sum(46 + len(nm) + (12 if x else 0) for nm, x in zip(names, extras))
            assert r.file[cd:cd + 4] == b"PK\x01\x02"
            done += 1
    return done


def zip64_count(target, counts=(65534, 65535, 65536)):
    """empty stored entries with 5-byte names: the locator is absent, present, present; zipfile lists the count"""
    done = 0
    for n in counts:
        names = [b"%05d" % i for i in range(n)]
        raws = [b""] * n
        r = target.write(raws, names, 4096, 0, name_shift=0)
        assert r.rc == 0 and r.status == 0 and r.guard_ok and r.total == n * (35 + 51) + (76 if n >= 0xFFFF else 0) + 22, r
        assert end_structure(r.file, 0, n) == (n >= 0xFFFF)
        with zipfile.ZipFile(io.BytesIO(r.file)) as zf:
            got = zf.namelist()
            assert len(got) == n and got[0] == "00000" and got[-1] == "%05d" % (n - 1)
        want = craft(raws, names, raws, 0)
        assert r.file == want.file and r.table == want.table and r.info == want.info
        done += 1
    return done


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------------------
def capacity(target, levels=(6, 0)):
    done = 0
    names = names_of(len(LENS_A))
    for level in levels:
        raws = entries_of("mix", LENS_A)
        full = target.write(raws, names, 4096, level)
        want = check_archive(target, full, raws, names, 4096, level, 0)
        total = full.total
        rows = [struct.unpack_from("<QQII", full.table, i * ROW) for i in range(len(raws))]
        # every unit of the archive: local header + name, the payload of a piece, central record, end record
        units, first = [], []
        for i, (data_off, name_off, csize, _) in enumerate(rows):
            first.append(len(units))
            units.append((data_off - 30 - len(names[i]), data_off))
            at = data_off
            for size in target.piece_sizes(raws[i], 4096, level, 0):
                units.append((at, at + size))
                at += size
            assert at == data_off + csize
        cen0 = len(units)
        for i, (data_off, name_off, csize, _) in enumerate(rows):
            units.append((name_off - 46, name_off + len(names[i])))
        units.append((total - 22, total))
        assert units[0][0] == 0 and all(a[1] == b[0] for a, b in zip(units, units[1:])) and units[-2][1] == total - 22
        r = target.write(raws, names, 4096, level, cap=total)
        assert (r.rc, r.status, r.total) == (0, 0, total) and r.guard_ok and r.buf == full.file
        h5, p5 = units[first[5]], units[first[5] + 2]        # the sixth entry's header and the second of its three pieces
        c3 = units[cen0 + 3]
        for cap in (total - 1, (p5[0] + p5[1]) // 2, h5[0] + 17, (c3[0] + c3[1]) // 2, 0):
            r = target.write(raws, names, 4096, level, cap=cap)
            assert (r.rc, r.status, r.total) == (0, Z_BUF_ERROR, total) and r.guard_ok, (cap, r)
            assert r.table == full.table and r.info == full.info
            for lo, hi in units:                            # a unit that ends at or before cap is right, one that crosses it untouched
                if hi <= cap:
                    assert r.buf[lo:hi] == full.file[lo:hi], (cap, lo, hi)
                else:
                    assert r.buf[lo:min(hi, cap)] == bytes([FILL]) * (min(hi, cap) - min(lo, cap)), (cap, lo, hi)
            done += 1
        assert want is None or want.file == full.file
    return done


# ---- 6. arguments --------------------------------------------------------------------------------------------------------------------------
EMPTY = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0, 0, 0, 0, 0)


def arguments(target):
    raws = entries_of("text", [700, 0, 4097])
    names = names_of(3)
    w = lambda **kw: target.write(raws, names, **{"pb": 4096, **kw})
    bad = [w(pb=0), w(pb=(1 << 30) + 1), w(level=10), w(level=-2), w(strategy=5), w(strategy=-1), w(in_bytes=(1 << 31) * 4096, cap=4096)]
    bad += [w(count=1 << 31, cap=4096), w(count=0xFFFFFFFF, cap=4096)]      # n_entries above 2^31 - 1: refused in front of every table
    bad += [w(null=k) for k in ("ctx", "in", "off", "len", "noff", "out", "olen", "st")]
    for i, r in enumerate(bad):
        assert r.rc == E_ARG, (i, r)
    assert int(target.L.zmi_zip_bound(3, 10, 1000, 0, 6)) == 0
    done = len(bad) + 1
    # the sum of the lengths above in_bytes: the table lives on the device, ZMI_E_ARG arrives in the status word, no entry is written
    r = w(in_bytes=sum(map(len, raws)) - 1)
    assert (r.rc, r.status, r.guard_ok, r.file) == (0, E_ARG, True, EMPTY), r
    assert struct.unpack("<QQQQQii", r.info) == (0, 0, 0, 0, 0, 0, 0)
    # a length above ZMI_ZIP_ENTRY_MAX: an empty entry
    for level in (6, 0):
        r = w(level=level, lens=[700, ENTRY_MAX + 1, 4097])
        assert (r.rc, r.status) == (0, E_ARG) and r.guard_ok, r
        r.status = 0
        check_archive(target, r, [raws[0], b"", raws[2]], names, 4096, level, 0)
        done += 1
    # no entries: the 22 bytes; d_entries / d_info NULL; level -1 is level 6; in_bytes may be generous
    for level in (6, 0, -1, 1, 9):
        r = target.write([], [], 4096, level)
        assert (r.rc, r.status, r.guard_ok, r.file) == (0, 0, True, EMPTY), (level, r)
        assert struct.unpack("<QQQQQii", r.info) == (0, 0, 0, 0, 0, 0, 0)
        done += 1
    ref = w()
    check_archive(target, ref, raws, names, 4096, 6, 0)
    for kw in ({"table": False}, {"info": False}, {"table": False, "info": False}, {"level": -1}, {"in_bytes": 100000}, {"cap": ref.total + 999}):
        r = w(**kw)
        assert (r.rc, r.status, r.guard_ok) == (0, 0, True) and r.file == ref.file, kw
        done += 1
    return done + 2


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------------
def entry_bytes(res, names):
    """name -> the entry's local header, name and payload bytes"""
    out = {}
    for i, nm in enumerate(names):
        data_off, _, csize, _ = struct.unpack_from("<QQII", res.table, i * ROW)
        out[nm] = res.file[data_off - 30 - len(nm):data_off + csize]
    return out


def determinism(target, levels=(0, 6, 9)):
    """an entry's bytes depend on its own bytes, piece_bytes, level and strategy alone; two calls give equal archives"""
    done = 0
    names = names_of(len(LENS_A))
    extra_names = [b"more/%d" % i for i in range(5)]
    for level in levels:
        raws = entries_of("mix", LENS_A)
        a, b = target.write(raws, names, 4096, level), target.write(raws, names, 4096, level)
        assert a.rc == 0 and a.status == 0 and a.file == b.file and a.table == b.table and a.info == b.info
        ref = entry_bytes(a, names)
        order = [4, 0, 6, 2, 5, 1, 3]
        more = entries_of("text", [5000, 0, 123, 9000, 4096], seed=40)
        for r, nms in ((target.write([raws[i] for i in order], [names[i] for i in order], 4096, level), [names[i] for i in order]),
                       (target.write(more[:2] + raws + more[2:], extra_names[:2] + names + extra_names[2:], 4096, level, in_bytes=1 << 16),
                        extra_names[:2] + names + extra_names[2:]),
                       (target.write(raws, names, 4096, level, shift=7, scattered=True, name_shift=0), names)):
            assert r.rc == 0 and r.status == 0 and r.guard_ok, r
            got = entry_bytes(r, nms)
            assert all(got[nm] == ref[nm] for nm in names)
            done += 1
    return done
