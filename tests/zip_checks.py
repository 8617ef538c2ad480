"""Checks of the ZIP reader (zmi_zip_directory_dev / zmi_zip_inflate_dev, include/zmi355.h), shared by tests/test_emu_zip.py (CPU, the
emulator build) and tests/test_gpu_zip.py (the MI355X), both through the C ABI on buffers a `mem` object owns (put / full / read /
stream, as in tests/bgzf_checks.py).

The judges are Python's zipfile and zlib.  Archives come from zipfile itself or from the crafter below (struct.pack), which can force
ZIP64 records, every subset of the three ZIP64 extra values, prefixes, comments, local names and extras that differ from the central
ones, and wrong fields.  Every VALID crafted archive first passes zipfile.ZipFile(...).testzip() is None with equal contents
(`pinned`), so the crafter itself is pinned.  Two kinds of valid archive zipfile cannot judge -- it takes the LAST end-record signature,
so one spelled inside the archive comment fools it, and it refuses a local name that differs from the central one -- are judged by the
crafter's own entry list."""
import ctypes as C
import functools
import io
import random
import struct
import zipfile
import zlib

import numpy as np

Z_DATA_ERROR, Z_BUF_ERROR, Z_VERSION_ERROR, E_ARG = -3, -5, -6, -103
ZA_NOEOCD, ZA_BOUNDS, ZA_CHAIN, ZA_COUNT, ZA_ZIP64, ZA_MULTIDISK = 1, 2, 3, 4, 5, 6
ZE_LOCAL, ZE_METHOD, ZE_CRYPT, ZE_BIG, ZE_EXTRA, ZE_STORED, ZE_DATA, ZE_LENGTH, ZE_CHECK, ZE_OUT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
GUARD, FILL = 64, 0xC7
CANARY = 0x77
ENTRY = np.dtype([("data_off", "<u8"), ("name_off", "<u8"), ("csize", "<u4"), ("usize", "<u4"), ("crc32", "<u4"), ("dos_time", "<u4"),
                  ("ext_attr", "<u4"), ("method", "<u2"), ("flags", "<u2"), ("name_len", "<u2"), ("reserved", "<u2"), ("status", "<i4")])
INFO = np.dtype([("n_entries", "<u8"), ("n_listed", "<u8"), ("cd_off", "<u8"), ("cd_size", "<u8"), ("base", "<u8"), ("status", "<i4"),
                 ("detail", "<i4")])
assert ENTRY.itemsize == 48 and INFO.itemsize == 48
SHIFTS = [0, 1, 3, 15]


def bind(L):
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_zip_walk_tile.restype = u32
    L.zmi_zip_walk_tile.argtypes = []
    L.zmi_zip_directory_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_zip_inflate_dev.argtypes = [vp, vp, u64, vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    return L


# ---- data -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text(n, seed=1):
    r = random.Random(seed)
    words = [bytes(r.randrange(97, 123) for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + (b" " if r.random() < 0.9 else bytes([r.randrange(256)]))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def noise(n, seed=1):
    return np.random.RandomState(seed).bytes(n)


def raw_deflate(data, level=6, strategy=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


# ---- the crafter ------------------------------------------------------------------------------------------------------------------------
class Ent:
    """One entry.  The defaults make a valid entry; every keyword overrides one written field (c_*: central, l_*: local)."""

    def __init__(self, name, data=b"", method=8, level=6, strategy=0, **kw):
        self.name = name if isinstance(name, bytes) else name.encode("utf-8")
        self.data = data
        self.method = method
        self.payload = kw.pop("payload", None)
        if self.payload is None:
            self.payload = raw_deflate(data, level, strategy) if method == 8 else data
        self.crc = zlib.crc32(data)
        self.flags = kw.pop("flags", 0)
        self.z64 = kw.pop("z64", "")                     # which of usize / csize / offset stand in the ZIP64 extra: a subset of "uco"
        self.comment = kw.pop("comment", b"")
        self.c_extra = kw.pop("c_extra", b"")
        self.l_extra = kw.pop("l_extra", b"")
        self.l_name = kw.pop("l_name", None)
        self.time, self.date = kw.pop("time", 0x6A3B), kw.pop("date", 0x5B21)
        self.ext_attr = kw.pop("ext_attr", 0o644 << 16)
        self.fix = kw                                    # c_crc c_csize c_usize c_method c_sig c_off c_disk l_sig l_method l_flags l_zero
        self.expect = (0, 0)                             # what a slot that reads it reports: (status, detail)


def craft(entries, comment=b"", prefix=b"", zip64=False, trailing=b"", **fix):
    """-> the archive's bytes.  fix: count, cd_size_add, disk, z64_size, z64_count, z64_disk, loc_disk"""
    out = bytearray(prefix)
    cen = bytearray()
    for e in entries:
        f = e.fix
        off = len(out) - len(prefix)
        l_name = e.name if e.l_name is None else e.l_name
        zero = f.get("l_zero", False)                    # general-purpose bit 3: the local header holds zeros
        out += struct.pack("<IHHHHHIIIHH", f.get("l_sig", 0x04034B50), 20, f.get("l_flags", e.flags), f.get("l_method", e.method), e.time, e.date,
                           0 if zero else e.crc, 0 if zero else len(e.payload), 0 if zero else len(e.data), len(l_name), len(e.l_extra))
        out += l_name + e.l_extra + e.payload
        usize, csize, loff = f.get("c_usize", len(e.data)), f.get("c_csize", len(e.payload)), f.get("c_off", off)
        vals = b""
        fu, fc, fo = usize, csize, loff
        if "u" in e.z64:
            vals, fu = vals + struct.pack("<Q", usize), 0xFFFFFFFF
        if "c" in e.z64:
            vals, fc = vals + struct.pack("<Q", csize), 0xFFFFFFFF
        if "o" in e.z64:
            vals, fo = vals + struct.pack("<Q", loff), 0xFFFFFFFF
        c_extra = (struct.pack("<HH", 1, len(vals)) + vals if e.z64 else b"") + e.c_extra
        if "c_extra_raw" in f:
            c_extra = f["c_extra_raw"]
        cen += struct.pack("<IHHHHHHIIIHHHHHII", f.get("c_sig", 0x02014B50), 0x0314, 45 if e.z64 else 20, e.flags, f.get("c_method", e.method),
                           e.time, e.date, f.get("c_crc", e.crc), fc, fu, len(e.name), len(c_extra), len(e.comment), f.get("c_disk", 0), 0,
                           e.ext_attr, fo)
        cen += e.name + c_extra + e.comment
    cd_off, n = len(out) - len(prefix), len(entries)
    out += cen
    count = fix.get("count", n)
    cd_size = len(cen) + fix.get("cd_size_add", 0)
    if zip64:
        out += struct.pack("<IQHHIIQQQQ", 0x06064B50, fix.get("z64_size", 44), 45, 45, fix.get("z64_disk", 0), 0, n, fix.get("z64_count", n),
                           cd_size, cd_off)
        out += struct.pack("<IIQI", 0x07064B50, fix.get("loc_disk", 0), cd_off + len(cen), 1)
        out += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(count, 0xFFFF), min(count, 0xFFFF), 0xFFFFFFFF, 0xFFFFFFFF, len(comment))
    else:
        out += struct.pack("<IHHHHIIH", 0x06054B50, fix.get("disk", 0), 0, count & 0xFFFF, count & 0xFFFF, cd_size, cd_off, len(comment))
    return bytes(out + comment + trailing)


def pinned(blob, entries):
    """the crafter's pin: zipfile reads the archive, every CRC holds, the contents are the entries'"""
    zf = zipfile.ZipFile(io.BytesIO(blob))
    assert zf.testzip() is None
    infos = zf.infolist()
    assert len(infos) == len(entries)
    for zi, e in zip(infos, entries):
        assert zf.read(zi) == e.data, zi.filename
    return blob


def mixed(n, big=True, seed=0):
    """n entries mixing stored, levels 1 / 6 / 9, Z_FIXED and incompressible bytes, of sizes 0 .. 3000, one of 300 000 bytes"""
    ents = []
    for i in range(n):
        size = (i * 733 + seed * 31) % 3001
        if big and i == 1:
            size = 300000
        kind = i % 6
        if kind == 0:
            ents.append(Ent("s/%d.txt" % i, text(size, i + 1), method=0))
        elif kind == 4:
            ents.append(Ent("f/%d.txt" % i, text(size, i + 1), strategy=zlib.Z_FIXED))
        elif kind == 5:
            ents.append(Ent("r/%d.bin" % i, noise(size, i + 1)))
        else:
            ents.append(Ent("t/%d.txt" % i, text(size, i + 1), level=(1, 6, 9)[kind - 1]))
    return ents


# ---- the target -------------------------------------------------------------------------------------------------------------------------
class Dir:
    def __init__(self, rc, info, entries, canary_ok, h_in, n, h_ent):
        self.rc, self.info, self.entries, self.canary_ok, self.h_in, self.n, self.h_ent = rc, info, entries, canary_ok, h_in, n, h_ent

    @property
    def status(self):
        return int(self.info["status"]), int(self.info["detail"]) & 0xFF

    @property
    def listed(self):
        return self.entries[:int(self.info["n_listed"])]


class Read:
    def __init__(self, rc, off, length, status, detail, out, clean):
        self.rc, self.off, self.len, self.status, self.detail, self.out, self.clean = rc, off, length, status, detail, out, clean

    def slot(self, j):
        return self.out[self.off[j]:self.off[j] + self.len[j]]


class Target:
    def __init__(self, L, ctx, mem):
        self.L, self.ctx, self.mem = bind(L), ctx, mem
        self.tile = int(self.L.zmi_zip_walk_tile())

    def directory(self, blob, cap=None, shift=0, ctx="ctx"):
        """one zmi_zip_directory_dev call; one entry of canary stands behind the `cap` the call owns"""
        m, n = self.mem, len(blob)
        if cap is None:
            cap = max(0, (n - 22) // 76)
        h_in = m.put(np.frombuffer(bytes(blob) + b"\0" * 16, dtype=np.uint8), shift)
        h_ent = m.full((cap + 1) * 48, CANARY)
        h_info = m.full(48, CANARY)
        rc = self.L.zmi_zip_directory_dev(self.ctx if ctx == "ctx" else ctx, h_in.ptr, n, h_ent.ptr, cap, h_info.ptr, m.stream)
        if rc != 0:
            return Dir(rc, None, None, True, h_in, n, h_ent)
        info = m.read(h_info, INFO)[0]
        ent = m.read(h_ent, ENTRY)
        canary_ok = bytes(ent[cap:].tobytes()) == bytes([CANARY]) * 48
        return Dir(rc, info, ent[:cap], canary_ok, h_in, n, h_ent)

    def inflate(self, d, sel=None, n_sel=None, align=1, cap=None, n_entries=None, null=None, ctx="ctx"):
        """one zmi_zip_inflate_dev call on the directory `d`; cap None: exactly the room the selection needs"""
        m = self.mem
        n_entries = int(d.info["n_listed"]) if n_entries is None else n_entries
        if n_sel is None:
            n_sel = n_entries if sel is None else len(sel)
        plan_off, plan_size = plan(d.entries[:n_entries], sel, n_sel, align)
        need = plan_off[-1]
        if cap is None:
            cap = need
        h_sel = m.put(np.array(list(sel) + [0], dtype=np.uint32)) if sel is not None else None
        h_out = m.full(GUARD + cap + GUARD, FILL)
        h_off = m.full((n_sel + 2) * 8, CANARY)
        h_len = m.full((n_sel + 1) * 4, CANARY)
        h_st = m.full((n_sel + 1) * 4, CANARY)
        h_det = m.full((n_sel + 1) * 4, CANARY)
        args = dict(off=h_off.ptr, len=h_len.ptr, st=h_st.ptr, det=h_det.ptr)
        if null:
            args[null] = None
        rc = self.L.zmi_zip_inflate_dev(self.ctx if ctx == "ctx" else ctx, d.h_in.ptr, d.n, d.h_ent.ptr, n_entries, h_sel.ptr if h_sel else None,
                                        n_sel, align, h_out.ptr + GUARD, cap, args["off"], args["len"], args["st"], args["det"], m.stream)
        if rc != 0:
            return Read(rc, None, None, None, None, None, True)
        off = [int(x) for x in m.read(h_off, np.uint64)]
        ln = [int(x) for x in m.read(h_len, np.uint32)]
        st = [int(x) for x in m.read(h_st, np.int32)]
        det = [int(x) for x in m.read(h_det, np.int32)]
        buf = m.read(h_out, np.uint8)
        word = int.from_bytes(bytes([CANARY]) * 8, "little")
        assert off[n_sel + 1] == word and ln[n_sel] == word & 0xFFFFFFFF, "the call wrote behind its tables"
        # untouched: the guards and every byte that lies in no planned region that fits (gaps, the room behind the last region)
        touched = np.zeros(cap, dtype=bool)
        for j in range(n_sel):
            if plan_off[j] + plan_size[j] <= cap:
                touched[plan_off[j]:plan_off[j] + plan_size[j]] = True
        body = buf[GUARD:GUARD + cap]
        clean = bool((buf[:GUARD] == FILL).all() and (buf[GUARD + cap:] == FILL).all() and (body[~touched] == FILL).all())
        r = Read(rc, off[:n_sel + 1], ln[:n_sel], st[:n_sel], det[:n_sel], body.tobytes(), clean)
        r.plan_off, r.need = plan_off, need
        return r


def plan(entries, sel, n_sel, align):
    """the offsets the contract gives: the usize of the readable slots in front, each rounded up to align; then the need"""
    off, sizes, at = [], [], 0
    align = align if 1 <= align <= 4096 and not align & (align - 1) else 1      # (a call that is refused plans nothing)
    for j in range(n_sel):
        k = j if sel is None else sel[j]
        size = int(entries[k]["usize"]) if k < len(entries) and int(entries[k]["status"]) == 0 else 0
        off.append(at)
        sizes.append(size)
        at += -(-size // align) * align
    return off + [at], sizes


# ---- judges -----------------------------------------------------------------------------------------------------------------------------
def check_against_zipfile(d, blob, base=0):
    """every listed entry against zipfile's ZipInfo, the name bytes and data_off against the archive itself"""
    infos = zipfile.ZipFile(io.BytesIO(blob)).infolist()
    assert d.rc == 0 and d.status == (0, 0) and d.canary_ok, (d.rc, d.status)
    assert int(d.info["n_entries"]) == len(infos) and int(d.info["base"]) == base
    for e, zi in zip(d.listed, infos):
        assert (int(e["usize"]), int(e["csize"]), int(e["crc32"]), int(e["method"]), int(e["flags"])) == \
               (zi.file_size, zi.compress_size, zi.CRC, zi.compress_type, zi.flag_bits), zi.filename
        y, mo, dd, hh, mi, ss = zi.date_time
        assert int(e["dos_time"]) == ((y - 1980) << 9 | mo << 5 | dd) << 16 | (hh << 11 | mi << 5 | ss // 2)
        assert int(e["ext_attr"]) == zi.external_attr and int(e["reserved"]) == 0
        name = blob[int(e["name_off"]):int(e["name_off"]) + int(e["name_len"])]
        assert name.decode("utf-8" if zi.flag_bits & 0x800 else "cp437") == zi.orig_filename
        nl, el = struct.unpack_from("<HH", blob, zi.header_offset + 26)
        assert int(e["data_off"]) == zi.header_offset + 30 + nl + el
    return infos


def check_read(r, want, sel=None):
    """want[k] = (status, detail, data) of a slot that reads entry k; every slot, the offsets, the need, and nothing written elsewhere"""
    assert r.rc == 0 and r.clean, (r.rc, r.clean)
    assert r.off == r.plan_off, (r.off[:8], r.plan_off[:8])
    for j in range(len(r.status)):
        k = j if sel is None else sel[j]
        st, det, data = want[k] if k < len(want) else (E_ARG, 0, b"")
        assert (r.status[j], r.detail[j]) == (st, det), (j, k, r.status[j], r.detail[j], st, det)
        if st == 0:
            assert r.len[j] == len(data) and r.slot(j) == data, (j, k)
        else:
            assert r.len[j] == 0, (j, k)


def good(entries):
    return [(e.expect[0], e.expect[1], e.data if e.expect[0] == 0 else b"") for e in entries]


def roundtrip(t, blob, entries, shift=0, align=1, base=0, judge_zipfile=True):
    """directory and full read of a valid archive"""
    d = t.directory(blob, shift=shift)
    if judge_zipfile:
        check_against_zipfile(d, blob, base)
    assert d.rc == 0 and d.status == (0, 0) and d.canary_ok and int(d.info["n_entries"]) == len(entries) == int(d.info["n_listed"])
    r = t.inflate(d, align=align)
    check_read(r, good(entries))
    return d, r


def judge_deflate(payload, usize, crc):
    """what zlib.decompressobj(-15) and zlib.crc32 say of a payload that must give usize bytes with that CRC-32 and end exactly"""
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(payload, usize + 1)
        while not d.eof and len(raw) <= usize and d.unconsumed_tail:
            more = d.decompress(d.unconsumed_tail, usize + 1 - len(raw))
            if not more and not d.eof:
                break
            raw += more
    except zlib.error:
        return Z_DATA_ERROR, ZE_DATA
    if not d.eof or d.unused_data or len(raw) != usize:
        return Z_DATA_ERROR, ZE_LENGTH
    if zlib.crc32(raw) != crc:
        return Z_DATA_ERROR, ZE_CHECK
    return 0, 0


# ---- 1. shapes --------------------------------------------------------------------------------------------------------------------------
def small_shapes(t):
    """the empty archive; one entry of 0 and of 1 byte, stored and deflated; a directory entry"""
    d = t.directory(craft([]))
    assert d.rc == 0 and d.status == (0, 0) and int(d.info["n_entries"]) == 0 == int(d.info["n_listed"]) and d.n == 22
    r = t.inflate(d)
    assert r.rc == 0 and r.off == [0] and r.clean
    n = 1
    for data in (b"", b"x"):
        for method in (0, 8):
            ents = [Ent("one", data, method=method)]
            roundtrip(t, pinned(craft(ents), ents), ents)
            n += 1
    ents = [Ent("d/", b"", method=0, ext_attr=0o40755 << 16 | 0x10), Ent("d/a", b"inside")]
    roundtrip(t, pinned(craft(ents), ents), ents)
    return n + 1


def shapes(t, counts=(3, 64, 65, 300), shifts=SHIFTS, aligns=(1, 16, 4096)):
    """mixed archives at every input alignment and output alignment: bytes, offsets, lengths, all status 0, nothing written in the
    gaps or behind out_cap"""
    n = 0
    for count in counts:
        ents = mixed(count)
        blob = pinned(craft(ents), ents)
        for k, shift in enumerate(shifts):
            roundtrip(t, blob, ents, shift=shift, align=aligns[k % len(aligns)])
            n += 1
        for align in aligns[len(shifts):]:
            roundtrip(t, blob, ents, align=align)
            n += 1
    return n


# ---- 2. the end record --------------------------------------------------------------------------------------------------------------------
def end_record(t):
    ents = mixed(4, big=False)
    n = 0
    for clen in (0, 1, 65535):
        comment = bytes((i * 7 + 1) % 251 for i in range(clen))
        roundtrip(t, pinned(craft(ents, comment=comment), ents), ents)
        n += 1
    # an end record spelled inside the comment (count 0, no comment of its own, more comment behind it): zipfile takes it and sees an
    # empty archive; the real record is the one whose comment ends the file
    fake = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0, 0, 0, 0, 0)
    blob = craft(ents, comment=b"see: " + fake + b" -- the end")
    assert len(zipfile.ZipFile(io.BytesIO(blob)).infolist()) == 0           # (the behaviour this case relies on)
    roundtrip(t, blob, ents, judge_zipfile=False)
    n += 1
    d = t.directory(craft(ents, trailing=b"\n"))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_NOEOCD) and int(d.info["n_entries"]) == 0 == int(d.info["n_listed"]) and d.canary_ok
    empty = craft([])
    for cut in (0, 21):
        d = t.directory(empty[:cut], cap=4)
        assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_NOEOCD) and d.canary_ok, cut
    d = t.directory(empty, cap=4)
    assert d.rc == 0 and d.status == (0, 0) and int(d.info["n_entries"]) == 0
    n += 4
    for plen in (1, 1000):
        prefix = noise(plen, 9)
        blob = craft(ents, prefix=prefix)
        zipfile.ZipFile(io.BytesIO(blob)).testzip()
        d, _ = roundtrip(t, blob, ents, base=plen, shift=plen % 16)
        assert int(d.info["base"]) == plen and int(d.entries[0]["data_off"]) == plen + 30 + len(ents[0].name)
        n += 1
    return n


# ---- 3. the chain across the walk's windows -------------------------------------------------------------------------------------------------
def _dir_start(blob):
    return zipfile.ZipFile(io.BytesIO(blob)).start_dir


def chain_edges(t, ss=range(46)):
    """the second directory entry starts s bytes in front of the end of the walk's first window, which begins at the 16-byte line of the
    directory's first byte: run with the directory on such a line (the header straddles the edge at byte 46 - s) and one byte off it"""
    T, n = t.tile, 0
    for s in ss:
        first = Ent("a", b"first")
        pad = T - s - (46 + len(first.name))
        first.comment = bytes(pad)
        ents = [first, Ent("b", text(200, 2)), Ent("c", text(70, 3), method=0)]
        blob = pinned(craft(ents), ents)
        start = _dir_start(blob)
        for shift in ((-start) % 16, (1 - start) % 16):
            roundtrip(t, blob, ents, shift=shift)
            n += 1
    return n


def false_guesses(t):
    """50 4b 01 02 spelled inside comments, names and extras, so that the first signature of a stretch of the directory is not where the
    chain enters it: behind a window's edge inside a long comment, as a whole fake entry, and in every name of an archive"""
    T, n = t.tile, 0
    fake = struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 20, 20, 0, 0, 0, 0, 0, 5, 5, 3, 0, 0, 0, 0, 0, 0) + b"abc"
    for at in (T - 2, T, T + 10, 2 * T + 5):
        first = Ent("a", b"first")
        first.comment = bytes(at - 47) + fake + b"PK\x01\x02" + bytes(T // 2)
        ents = [first, Ent("b", text(200, 2)), Ent("c", text(70, 3), method=0)] + mixed(3, big=False)
        blob = pinned(craft(ents), ents)
        start = _dir_start(blob)
        for shift in ((-start) % 16, (5 - start) % 16):
            roundtrip(t, blob, ents, shift=shift)
            n += 1
    ents = [Ent(b"PK\x01\x02%04d" % i, text(50 + i % 40, i), c_extra=struct.pack("<HH", 0x4B50, 4) + b"PK\x01\x02", comment=b"x" * (i % 97))
            for i in range(600)]
    blob = pinned(craft(ents), ents)
    roundtrip(t, blob, ents)
    return n + 1


def long_entry(t):
    """name, extra and comment of 65 535 bytes each, ordinary entries in front of it and behind it"""
    extra = struct.pack("<HH", 0x7777, 65531) + bytes(65531)
    ents = [Ent("in front", text(300, 1)), Ent(b"n" * 65535, text(500, 2), c_extra=extra, comment=b"c" * 65535), Ent("behind", text(100, 3)),
            Ent("last", b"z" * 40, method=0)]
    blob = pinned(craft(ents), ents)
    roundtrip(t, blob, ents)
    return 1


def directory_sizes(t):
    """directories of T - 1, T and T + 1 bytes"""
    T, n = t.tile, 0
    for size in (T - 1, T, T + 1):
        ents = mixed(5, big=False)
        fixed = sum(46 + len(e.name) for e in ents)
        ents[-1].comment = bytes(size - fixed)
        blob = pinned(craft(ents), ents)
        start = _dir_start(blob)
        d, _ = roundtrip(t, blob, ents, shift=(-start) % 16)
        assert int(d.info["cd_size"]) == size
        n += 1
    return n


# ---- 4. ZIP64 -------------------------------------------------------------------------------------------------------------------------------
def zip64_extras(t):
    """all 8 subsets of the extra's values on small entries, then the forced ZIP64 end record, then a version-2 record"""
    n = 0
    for mask in range(8):
        z64 = "".join(ch for b, ch in enumerate("uco") if mask >> b & 1)
        ents = [Ent("plain", text(100, 1)), Ent("z64", text(900, 2), z64=z64), Ent("stored", text(50, 3), method=0, z64=z64)]
        roundtrip(t, pinned(craft(ents), ents), ents)
        n += 1
    ents = mixed(3, big=False)
    blob = pinned(craft(ents, zip64=True), ents)
    d, _ = roundtrip(t, blob, ents)
    assert int(d.info["cd_off"]) == _dir_start(blob)
    blob = pinned(craft(ents, zip64=True, prefix=b"#!/bin/sh\n"), ents)
    roundtrip(t, blob, ents, base=10)
    d = t.directory(craft(ents, zip64=True, z64_size=44 + 12))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_ZIP64) and int(d.info["n_listed"]) == 0
    d = t.directory(craft(ents, zip64=True, z64_count=4))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_COUNT) and int(d.info["n_entries"]) == 3
    return n + 4


# ---- 5. local headers that differ from the directory -------------------------------------------------------------------------------------
class _Unseekable:
    def __init__(self):
        self.b = io.BytesIO()

    def write(self, data):
        return self.b.write(data)

    def flush(self):
        pass


def local_differs(t):
    n = 0
    # zipfile's force_zip64: a 20-byte local extra, a central extra of length 0
    b = io.BytesIO()
    datas = [text(700, 1), noise(300, 2), b""]
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as zf:
        for i, data in enumerate(datas):
            with zf.open("f%d" % i, "w", force_zip64=True) as f:
                f.write(data)
    blob = b.getvalue()
    assert struct.unpack_from("<H", blob, 28)[0] == 20 and struct.unpack_from("<H", blob, _dir_start(blob) + 30)[0] == 0
    n += _zipfile_roundtrip(t, blob, datas)
    # an unseekable writer: bit 3, zeros in the local header, a data descriptor behind the data
    u = _Unseekable()
    with zipfile.ZipFile(u, "w", zipfile.ZIP_DEFLATED) as zf:
        for i, data in enumerate(datas):
            zf.writestr("g%d" % i, data)
    blob = u.b.getvalue()
    assert struct.unpack_from("<H", blob, 6)[0] & 8 and struct.unpack_from("<II", blob, 18) == (0, 0)
    n += _zipfile_roundtrip(t, blob, datas)
    # crafted: the same with the crafter, and a local extra the directory does not have
    ents = [Ent("a", text(400, 4), flags=8, l_zero=True), Ent("b", text(90, 5), l_extra=struct.pack("<HH", 0x5455, 5) + b"\x01abcd"),
            Ent("c", b"tail", method=0)]
    roundtrip(t, pinned(craft(ents), ents), ents)
    # a local NAME of another length: zipfile refuses the archive ("File name in directory and header differ"), the judge is the list
    ents = [Ent("a", text(400, 4)), Ent("central-name", text(90, 5), l_name=b"loc"), Ent("c", b"tail", method=0)]
    roundtrip(t, craft(ents), ents, judge_zipfile=False)
    return n + 2


def _zipfile_roundtrip(t, blob, datas):
    d = t.directory(blob)
    check_against_zipfile(d, blob)
    r = t.inflate(d)
    check_read(r, [(0, 0, data) for data in datas])
    return 1


# ---- 6. flagged entries among good ones ---------------------------------------------------------------------------------------------------
def flagged(t):
    """in each archive one entry the directory flags: its slot's status and detail, length 0, and every other slot's bytes right"""
    n = 0

    def run(ents, k, reason, blob=None, usize=None):
        nonlocal n
        ents[k].expect = (Z_VERSION_ERROR, reason)
        blob = craft(ents) if blob is None else blob
        d = t.directory(blob)
        assert d.rc == 0 and d.status == (0, 0) and int(d.info["n_listed"]) == len(ents) and d.canary_ok
        st = [int(e["status"]) for e in d.listed]
        assert st == [reason if i == k else 0 for i in range(len(ents))], (st, k, reason)
        e = d.listed[k]
        assert blob[int(e["name_off"]):int(e["name_off"]) + int(e["name_len"])] == ents[k].name      # flagged, and still listed with its name
        if usize is not None:
            assert int(e["usize"]) == usize
        check_read(t.inflate(d), good(ents))
        check_read(t.inflate(d, sel=[k, 0, k]), good(ents), sel=[k, 0, k])
        n += 1

    def base():
        return [Ent("a", text(1000, 1)), Ent("b", text(500, 2)), Ent("c", text(200, 3), method=0), Ent("d", text(800, 4))]

    # zipfile's own bzip2 and lzma entries
    for method, ze in ((zipfile.ZIP_BZIP2, 12), (zipfile.ZIP_LZMA, 14)):
        b = io.BytesIO()
        with zipfile.ZipFile(b, "w") as zf:
            zf.writestr("a", text(1000, 1), zipfile.ZIP_DEFLATED)
            zf.writestr("b", text(500, 2), method)
            zf.writestr("c", text(200, 3), zipfile.ZIP_STORED)
        ents = [Ent("a", text(1000, 1)), Ent("b", text(500, 2)), Ent("c", text(200, 3), method=0)]
        run(ents, 1, ZE_METHOD, blob=b.getvalue())
        assert ze == method
    ents = base()
    ents[1] = Ent("b", text(500, 2), method=9)
    run(ents, 1, ZE_METHOD)
    ents = base()
    ents[2] = Ent("c", text(200, 3), method=0, flags=1)
    run(ents, 2, ZE_CRYPT)
    ents = base()
    ents[0] = Ent("a", text(1000, 1), flags=0x40)
    run(ents, 0, ZE_CRYPT)
    ents = base()
    ents[1] = Ent("b", text(500, 2), z64="u", c_usize=(1 << 32) + 5)
    run(ents, 1, ZE_BIG, usize=0xFFFFFFFF)
    ents = base()
    ents[2] = Ent("c", text(200, 3), method=0, c_usize=199)
    run(ents, 2, ZE_STORED)
    ents = base()
    ents[1] = Ent("b", text(500, 2), l_sig=0x04034B51)
    run(ents, 1, ZE_LOCAL)
    ents = base()
    ents[3] = Ent("d", text(800, 4), c_off=1 << 20)                  # a local header behind the file
    run(ents, 3, ZE_LOCAL)
    ents = base()
    ents[3] = Ent("d", text(800, 4), c_csize=len(raw_deflate(text(800, 4))) + 1)     # the last entry's data reaches into the directory
    run(ents, 3, ZE_LOCAL)
    ents = base()
    ents[1] = Ent("b", text(500, 2), l_method=0)
    run(ents, 1, ZE_LOCAL)
    ents = base()
    ents[1] = Ent("b", text(500, 2), c_csize=0xFFFFFFFF)             # all ones and no ZIP64 extra
    run(ents, 1, ZE_EXTRA)
    ents = base()
    ents[1] = Ent("b", text(500, 2), c_usize=0xFFFFFFFF, c_extra_raw=struct.pack("<HHI", 1, 4, 7))   # an extra too short for its value
    run(ents, 1, ZE_EXTRA)
    return n


# ---- 7. corruption --------------------------------------------------------------------------------------------------------------------------
def corruption(t):
    """each on entry 2 of a 5-entry archive; the neighbours keep status 0 and their bytes"""
    n = 0
    data = text(5000, 7)
    payload = raw_deflate(data)
    crc = zlib.crc32(data)

    def run(entry, expect, accept=None):
        nonlocal n
        ents = [Ent("a", text(700, 1)), Ent("b", noise(300, 2), method=0), entry, Ent("d", text(900, 4), method=0), Ent("e", text(1200, 5))]
        entry.expect = expect
        d = t.directory(craft(ents))
        assert d.rc == 0 and d.status == (0, 0) and [int(e["status"]) for e in d.listed] == [0] * 5
        r = t.inflate(d, align=16)
        if accept is not None:
            assert (r.status[2], r.detail[2]) in accept, (r.status[2], r.detail[2], accept)
            entry.expect = (r.status[2], r.detail[2])
        check_read(r, good(ents))
        n += 1

    for at in (len(payload) // 3, len(payload) // 2, len(payload) - 2):
        bad = bytearray(payload)
        bad[at] ^= 0x10
        verdict = judge_deflate(bytes(bad), len(data), crc)
        assert verdict[0] == Z_DATA_ERROR
        run(Ent("x", data, payload=bytes(bad)), verdict)
    run(Ent("x", data, c_crc=crc ^ 1), (Z_DATA_ERROR, ZE_CHECK))
    run(Ent("x", data, method=0, c_crc=crc ^ 0x80000000), (Z_DATA_ERROR, ZE_CHECK))
    run(Ent("x", data, c_usize=len(data) - 1), (Z_DATA_ERROR, ZE_LENGTH))      # (check_read: nothing written behind the region)
    run(Ent("x", data, c_usize=len(data) + 1), (Z_DATA_ERROR, ZE_LENGTH))
    # csize one too large: the stream ends one byte early (the byte behind it is the next local header's 'P')
    run(Ent("x", data, c_csize=len(payload) + 1), (Z_DATA_ERROR, ZE_LENGTH))
    verdict = judge_deflate(payload[:-1], len(data), crc)
    assert verdict in ((Z_DATA_ERROR, ZE_DATA), (Z_DATA_ERROR, ZE_LENGTH))
    run(Ent("x", data, c_csize=len(payload) - 1), verdict)
    return n


# ---- 8. archive errors ---------------------------------------------------------------------------------------------------------------------
def archive_errors(t):
    ents = mixed(4, big=False)
    d = t.directory(craft(ents, cd_size_add=1))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_BOUNDS) and int(d.info["n_listed"]) == 0 and d.canary_ok
    bad = mixed(4, big=False)
    bad[2].fix["c_sig"] = 0x02014B51
    d = t.directory(craft(bad))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_CHAIN) and int(d.info["detail"]) >> 8 == 2
    assert int(d.info["n_listed"]) == 2 == int(d.info["n_entries"]) and [int(e["status"]) for e in d.listed] == [0, 0]
    check_read(t.inflate(d), good(ents[:2]))                         # the good entries in front of the break are readable
    d = t.directory(craft(ents, count=5))
    assert d.rc == 0 and d.status == (Z_DATA_ERROR, ZA_COUNT) and int(d.info["n_entries"]) == 4
    d = t.directory(craft(ents, disk=1))
    assert d.rc == 0 and d.status == (Z_VERSION_ERROR, ZA_MULTIDISK) and int(d.info["n_listed"]) == 0
    d = t.directory(craft(ents, zip64=True, z64_disk=2))
    assert d.rc == 0 and d.status == (Z_VERSION_ERROR, ZA_MULTIDISK)
    bad = mixed(4, big=False)
    bad[1].fix["c_disk"] = 3
    d = t.directory(craft(bad))
    assert d.rc == 0 and d.status == (Z_VERSION_ERROR, ZA_MULTIDISK) and int(d.info["n_entries"]) == 4
    return 6


# ---- 9. selection and room ------------------------------------------------------------------------------------------------------------------
def selection(t):
    ents = mixed(7)
    blob = pinned(craft(ents), ents)
    d = t.directory(blob)
    want = good(ents)
    n = 0
    for sel in ([1, 3, 5], [6, 5, 4, 3, 2, 1, 0], [2, 2, 0, 2], [0, 7, 1, 4000000000, 2], []):
        for align in (1, 16):
            r = t.inflate(d, sel=sel, align=align)
            if sel:
                check_read(r, want, sel=sel)
            else:
                assert r.rc == 0 and r.off == [0] and r.clean
            n += 1
    full = t.inflate(d, align=16)
    check_read(full, want)
    need, end2 = full.need, full.off[2] + len(ents[2].data)
    for cap in (need, need - 1, end2, 0):
        r = t.inflate(d, align=16, cap=cap)
        assert r.rc == 0 and r.clean and r.off == full.off and r.off[-1] == need
        for j, e in enumerate(ents):
            if r.off[j] + len(e.data) <= cap:
                assert (r.status[j], r.detail[j], r.len[j]) == (0, 0, len(e.data)) and r.slot(j) == e.data, (cap, j)
            else:
                assert (r.status[j], r.detail[j], r.len[j]) == (Z_BUF_ERROR, ZE_OUT, 0), (cap, j)
        n += 1
    # a cap of fewer entries than the archive holds: the first are listed, n_entries tells the rest
    few = t.directory(blob, cap=3)
    assert few.rc == 0 and few.status == (0, 0) and few.canary_ok and int(few.info["n_entries"]) == 7 and int(few.info["n_listed"]) == 3
    check_read(t.inflate(few), want[:3])
    none = t.directory(blob, cap=0)
    assert none.rc == 0 and none.status == (0, 0) and int(none.info["n_entries"]) == 7 and int(none.info["n_listed"]) == 0
    return n + 2


def arguments(t):
    ents = mixed(3, big=False)
    d = t.directory(craft(ents))
    assert t.directory(craft(ents), ctx=None).rc == E_ARG
    assert t.inflate(d, ctx=None).rc == E_ARG
    for align in (0, 3, 8192):
        assert t.inflate(d, align=align).rc == E_ARG
    assert t.L.zmi_zip_inflate_dev(t.ctx, d.h_in.ptr, d.n, d.h_ent.ptr, 3, None, 3, 0, None, 0, None, None, None, None, t.mem.stream) == E_ARG
    assert t.inflate(d, null="off").rc == E_ARG
    assert t.inflate(d, null="st").rc == E_ARG
    check_read(t.inflate(d), good(ents))
    return 8


def determinism(t):
    """the same words and bytes whatever the alignment of d_in and the number of slots"""
    ents = mixed(20, big=False)
    blob = pinned(craft(ents), ents)
    d0 = t.directory(blob, shift=0)
    ref = t.inflate(d0)
    for shift in (1, 15):
        d = t.directory(blob, shift=shift)
        assert d.listed.tobytes() == d0.listed.tobytes() and d.info.tobytes() == d0.info.tobytes()
        r = t.inflate(d)
        assert (r.off, r.len, r.status, r.detail, r.out) == (ref.off, ref.len, ref.status, ref.detail, ref.out)
    for k in (0, 7, 19):
        one = t.inflate(d0, sel=[k])
        assert (one.status, one.detail, one.len) == ([0], [0], [len(ents[k].data)]) and one.slot(0) == ents[k].data
    return 5
