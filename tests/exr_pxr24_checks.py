"""Checks of OpenEXR PXR24 (compression 5) in the reader (zmi_exr_headers_dev / zmi_exr_read_dev) and the writer (zmi_exr_write_dev),
shared by tests/test_exr_pxr24_craft.py (CPU, no library: the judges against each other and against the pinned bytes of
include/zmi355.h), tests/test_emu_exr_pxr24.py (CPU, the emulator build) and tests/test_gpu_exr_pxr24.py (the MI355X).

No OpenEXR library stands behind these tests.  The judges are two pieces of code in this file, neither of them the code under test and
neither sharing code with the other: the forward transform `pxr24_forward` (loops over samples and bytes, `f24` as the header states
it; `pxr24_forward_fast` / `f24_fast` are its vectorised twins for large chunks, pinned against the loops by the craft test) and the
reference reader `pxr24_undo` (np.cumsum on widened integers, masking and slicing).  Files are crafted with exr_checks.Exr and injected
streams; the file's table and chunk headers are taken apart by exr_write_checks.chunks."""
import copy
import struct
import types
import zlib

import numpy as np

import exr_checks as X
import exr_write_checks as W
from exr_checks import (E_ARG, XE_CHUNK, XE_DATA, XE_LENGTH, XE_COMPRESSION, UINT, HALF, FLOAT, NONE, ZIPS, ZIP, ONE_HALF, RGBA, MIXED, SIZE, NP,
                        FILL, Exr)
from png_write_checks import EXACT, expected_offsets, zlib_header

PXR24 = 5
P = {UINT: 4, HALF: 2, FLOAT: 3}                                        # the bytes of a sample inside the stream
ONE_FLOAT, ONE_UINT = (("Z", FLOAT),), (("id", UINT),)
LAYOUTS = (ONE_HALF, RGBA, MIXED, ONE_FLOAT, ONE_UINT)


def bind(L):
    import ctypes as C
    W.bind(L)
    L.zmi_exr_pxr24_trip.restype, L.zmi_exr_pxr24_trip.argtypes = C.c_uint32, []
    return L


# ---- the forward judge: loops ---------------------------------------------------------------------------------------------------------------
def f24(u):
    """the 32 bits of a float -> its 24 bits, as include/zmi355.h states it"""
    s, e, m = u & 0x80000000, u & 0x7F800000, u & 0x007FFFFF
    if e == 0x7F800000:
        if m != 0:
            m >>= 8
            i = (e >> 8) | m | (1 if m == 0 else 0)
        else:
            i = e >> 8
    else:
        i = ((e | m) + (m & 0x80)) >> 8
        if i >= 0x7F8000:
            i = (e | m) >> 8
    return (s >> 8) | i


def pxr24_forward(raw, w, h, channels):
    """the raw bytes of a chunk of h rows of w pixels -> the bytes a PXR24 writer hands to zlib"""
    out, at = bytearray(), 0
    for _ in range(h):
        for _, t in channels:
            p, size = P[t], SIZE[t]
            planes = [bytearray(w) for _ in range(p)]
            prev = 0
            for x in range(w):
                v = int.from_bytes(raw[at + x * size:at + (x + 1) * size], "little")
                if t == FLOAT:
                    v = f24(v)
                diff = (v - prev) % (1 << (8 * p))
                prev = v
                for j in range(p):
                    planes[j][x] = (diff >> (8 * (p - 1 - j))) & 255
            for pl in planes:
                out += pl
            at += w * size
    assert at == len(raw)
    return bytes(out)


def f24_fast(u):
    """f24 on an array of uint32 (tests/test_exr_pxr24_craft.py pins it against the loop)"""
    u = np.asarray(u).astype(np.int64)
    s, e, m = u & 0x80000000, u & 0x7F800000, u & 0x007FFFFF
    nan = (e >> 8) | (m >> 8) | ((m >> 8) == 0).astype(np.int64)
    rnd = ((e | m) + (m & 0x80)) >> 8
    rnd = np.where(rnd >= 0x7F8000, (e | m) >> 8, rnd)
    special = e == 0x7F800000
    i = np.where(special, np.where(m != 0, nan, e >> 8), rnd)
    return ((s >> 8) | i).astype(np.uint32)


def pxr24_forward_fast(raw, w, h, channels):
    """the same bytes for large chunks"""
    per_px = sum(SIZE[t] for _, t in channels)
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, w * per_px)
    parts, col = [], 0
    for _, t in channels:
        run = np.ascontiguousarray(rows[:, col:col + w * SIZE[t]])
        col += w * SIZE[t]
        v = run.view("<u2" if t == HALF else "<u4").astype(np.int64)
        if t == FLOAT:
            v = f24_fast(v).astype(np.int64)
        prev = np.concatenate([np.zeros((h, 1), dtype=np.int64), v[:, :-1]], axis=1)
        diff = (v + (1 << 32) - prev) % (1 << (8 * P[t]))
        parts.append(np.concatenate([((diff >> (8 * (P[t] - 1 - j))) & 255).astype(np.uint8) for j in range(P[t])], axis=1))
    return np.concatenate(parts, axis=1).tobytes()


def forward(raw, w, h, channels):
    return pxr24_forward_fast(raw, w, h, channels) if len(raw) > 2048 else pxr24_forward(raw, w, h, channels)


# ---- the reference reader: np.cumsum, masking and slicing -------------------------------------------------------------------------------------
def pxr24_undo(d, w, h, channels):
    """the inflated bytes of a PXR24 chunk -> the raw bytes a reader returns (a FLOAT's low byte is 0)"""
    per_p = sum(P[t] for _, t in channels)
    assert len(d) == w * h * per_p, (len(d), w, h)
    a = np.frombuffer(d, dtype=np.uint8).reshape(h, w * per_p)
    out, col = [], 0
    for _, t in channels:
        p = P[t]
        word = np.zeros((h, w), dtype=np.int64)
        for j in range(p):
            word |= a[:, col + j * w:col + (j + 1) * w].astype(np.int64) << (8 * (p - 1 - j))
        col += p * w
        v = np.cumsum(word, axis=1) & ((1 << (8 * p)) - 1)
        if t == FLOAT:
            v = v << 8
        out.append(v.astype("<u2" if t == HALF else "<u4").view(np.uint8).reshape(h, -1))
    return np.concatenate(out, axis=1).tobytes()


def read_file(blob, p):
    """a written or crafted PXR24 file of the geometry of p -> (region with FILL in the gaps, [chunk stored raw]); the table and the
    chunk headers are judged by exr_write_checks.chunks"""
    planes = [np.zeros((p.height, p.width), dtype="<u2" if t == HALF else "<u4") for _, t in p.channels]
    stored = []
    for (size, data), (x0, y0, w, h), raw in zip(W.chunks(blob, p), p.boxes, p.raw):
        stored.append(size == len(raw))
        got = data if size == len(raw) else pxr24_undo(zlib.decompress(data), w, h, p.channels)
        rows = np.frombuffer(got, dtype=np.uint8).reshape(h, -1)
        col = 0
        for pl, (_, t) in zip(planes, p.channels):
            pl[y0:y0 + h, x0:x0 + w] = np.ascontiguousarray(rows[:, col:col + w * SIZE[t]]).view(pl.dtype)
            col += w * SIZE[t]
    return region_of(planes), stored


def region_of(planes):
    region = bytearray()
    for pl in planes:
        region += bytes([FILL]) * (-len(region) % 4)
        region += pl.tobytes()
    return bytes(region)


def lossy_region(p, stored):
    """the pixels of p with the FLOAT planes replaced by f24(..) << 8 in the chunks that are not stored raw"""
    planes = [pl.copy() for pl in p.planes]
    for (x0, y0, w, h), raw in zip(p.boxes, stored):
        if raw:
            continue
        for pl, (_, t) in zip(planes, p.channels):
            if t == FLOAT:
                bits = pl.view("<u4")
                bits[y0:y0 + h, x0:x0 + w] = f24_fast(bits[y0:y0 + h, x0:x0 + w]) << np.uint32(8)
    return region_of(planes)


# ---- the crafter ------------------------------------------------------------------------------------------------------------------------------
def craft(width, height, channels=MIXED, level=6, stream=None, **kw):
    """one PXR24 file: exr_checks.Exr built once for its raw chunks, then again with the zlib of the forward bytes wherever that is
    shorter than the raw chunk; stream: chunk -> data bytes placed instead (faults).  want = the region a reader must return."""
    if kw.get("planes") is None:
        kw["planes"] = [ramp(t, width, height, kw.get("seed", 1) + 11 * c) for c, (_, t) in enumerate(channels)]
    base = Exr(width, height, channels, PXR24, reference=False, **kw)
    st = {}
    for k, (raw, (x0, y0, w, h)) in enumerate(zip(base.raw, base.boxes)):
        z = zlib.compress(forward(raw, w, h, channels), level)
        if len(z) < len(raw):
            st[k] = z
    good = dict(st)
    st.update(stream or {})
    p = Exr(width, height, channels, PXR24, reference=False, stream=st, **kw)
    assert p.raw == base.raw
    p.want = lossy_region(p, [k not in good for k in range(p.n_chunks)])
    p.source = region_of(p.planes)
    return p


def source(p):
    """the object exr_write_checks.Target.write takes its pixels from: the layout of p, the pixels as they were"""
    q = copy.copy(p)
    q.want = p.source
    return q


def ramp(t, w, h, seed=0):
    """the smooth planes of exr_checks, the floats with bits below the 24 that PXR24 keeps"""
    pl = X.smooth_plane(t, w, h, seed)
    return (pl * np.float32(1.0000123)).astype("<f4") if t == FLOAT else pl


def palette(t, w, h, seed, k=4):
    """k random words with bits in every byte: every plane carries into the next and the differences wrap, and the chunk still shrinks"""
    rng = np.random.RandomState(seed)
    words = rng.randint(0, 1 << 32, k, dtype=np.int64).astype(np.uint32)
    if t == FLOAT:
        words &= np.uint32(0xFF7FFFFF)                                   # (finite)
    pick = words[rng.randint(0, k, (h, w))]
    return (pick & 0xFFFF).astype("<u2").view("<f2") if t == HALF else pick.astype("<u4").view(NP[t])


def all_ff(t, w, h):
    """every difference is ff..ff: v[x] = -(x + 1) mod 2^(8p) (FLOAT: negative NaNs whose 24 bits are exactly that)"""
    x = np.tile(np.arange(w, dtype=np.int64), (h, 1))
    v = ((1 << (8 * P[t])) - 1 - x) & ((1 << (8 * P[t])) - 1)
    if t == FLOAT:
        v = v << 8
    return v.astype("<u2").view("<f2") if t == HALF else v.astype("<u4").view(NP[t])


SPECIALS = np.array([0x7FC00000, 0x7F800001, 0x7F8000FF, 0xFF800080, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x000000FF,
                     0x807FFFFF, 0x80000000, 0x00000000, 0x3F8000FF, 0x3F800080, 0x3F80007F, 0x7F7FFF80, 0x7F7FFF7F], dtype=np.uint32)


def special_floats(w, h, seed):
    rng = np.random.RandomState(seed)
    return SPECIALS[rng.randint(0, len(SPECIALS), (h, w))].view("<f4")


class Target(W.Target):
    def __init__(self, L, ctx, mem):
        super().__init__(bind(L), ctx, mem)
        self.p24_trip = int(self.L.zmi_exr_pxr24_trip())


def widths_of(t):
    T = t.p24_trip
    return (1, 2, 3, 5, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)


# ---- reading ----------------------------------------------------------------------------------------------------------------------------------
def read_geometry(t, widths=None, heights=(1, 15, 16, 17, 33), layouts=LAYOUTS):
    """every width x height x layout in scanline files, one call per layout; every chunk of 64 pixels or more is compressed (ramps)"""
    n = 0
    for li, layout in enumerate(layouts):
        files = [craft(w, h, layout, seed=w + 3 * h + li, xmin=-(w % 3), ymin=-(h % 5)) for h in heights for w in (widths or widths_of(t))]
        assert all(not raw for p in files for raw, (x0, y0, w, h) in zip(p.stored, p.boxes) if w * h >= 64)   # (tiny chunks do not shrink)
        X.run(t.reader, files, align=16, shift=li)
        n += len(files)
    return n


def read_tiles(t, sizes=((16, 16), (32, 8))):
    """tiles on 37 x 21 and on exactly one tile, chunks physically shuffled, negative corners; three HALF channels of an odd W * H (the
    planes stand 2 bytes apart)"""
    files = []
    for tw, th in sizes:
        for layout in (RGBA, MIXED, ONE_FLOAT):
            files.append(craft(37, 21, layout, tile=(tw, th), order=2, seed=tw + len(layout), xmin=-5, ymin=-3))
        files.append(craft(tw, th, MIXED, tile=(tw, th), order=2, seed=th))
    files.append(craft(3, 3, RGBA[1:], seed=1))
    files.append(craft(33, 17, RGBA, seed=3, order=1))
    X.run(t.reader, files, align=16, shift=1)
    return len(files)


def read_values(t):
    """random words (a palette, so the chunks shrink), the FLOAT special values, and T + 1 pixels whose differences are all ff..ff"""
    T, files = t.p24_trip, []
    for li, layout in enumerate(LAYOUTS):
        w, h = 2 * T + 3, 5
        files.append(craft(w, h, layout, planes=[palette(ty, w, h, 7 * li + c) for c, (_, ty) in enumerate(layout)], seed=li))
        files.append(craft(T + 1, 2, layout, planes=[all_ff(ty, T + 1, 2) for _, ty in layout], seed=li))
    files.append(craft(T + 7, 3, ONE_FLOAT, planes=[special_floats(T + 7, 3, 5)], seed=1))
    files.append(craft(70, 20, MIXED, planes=[palette(HALF, 70, 20, 1), special_floats(70, 20, 6), palette(UINT, 70, 20, 2)], tile=(32, 8), seed=2))
    for p in files:
        assert not any(p.stored), (p.width, p.channels)
    X.run(t.reader, files, align=4, shift=2)
    return len(files)


def read_raw_chunks(t):
    """smooth chunks (compressed) and noise chunks (stored raw, full floats) side by side; a file of noise only"""
    a = craft(70, 50, RGBA, noise=(1, 3), seed=3)
    b = craft(37, 21, ONE_HALF, tile=(16, 16), noise=(2, 5), order=2, seed=5)
    c = craft(19, 20, RGBA, noise=(0, 1), seed=6)
    d = craft(40, 40, (("A", HALF), ("Z", FLOAT)), seed=8)
    d2 = craft(40, 40, (("A", HALF), ("Z", FLOAT)), seed=8, stream={1: d.raw[1]})          # a raw chunk that holds floats: they stay whole
    d2.want = lossy_region(d2, [False, True, False])
    assert a.stored == [False, True, False, True] and b.stored.count(True) == 2 and all(c.stored) and d2.stored == [False, True, False]
    for shift in (0, 1):
        X.run(t.reader, [a, b, c, d2], align=16, shift=shift)
    return 4


def read_faults(t):
    """each fault as file 1 of three, the neighbours still reading right"""
    def base(**kw):
        return craft(10, 40, MIXED, seed=21, **kw)

    good = base()
    x0, y0, w, h = good.boxes[1]
    n, d = len(good.raw[1]), forward(good.raw[1], w, h, MIXED)
    m = len(d)
    assert m < n and not any(good.stored)
    stream = zlib.compress(d)
    cases = []
    as_zip = zlib.compress(X.zip_forward(good.raw[1]))
    assert len(zlib.decompress(as_zip)) == n
    cases.append(("inflates to n", base(stream={1: as_zip}).fails(XE_LENGTH, 1)))
    cases.append(("one byte more than m", base(stream={1: zlib.compress(d + b"\0")}).fails(XE_LENGTH, 1)))
    cases.append(("one byte less than m", base(stream={2: zlib.compress(forward(good.raw[2], *good.boxes[2][2:], MIXED)[:-1])}).fails(XE_LENGTH, 2)))
    bad = bytearray(stream)
    bad[len(bad) // 2] ^= 0x10
    cases.append(("corrupt", base(stream={1: bytes(bad)}).fails(X.judge_stream(bytes(bad), m), 1)))
    adler = stream[:-4] + struct.pack(">I", zlib.adler32(d) ^ 1)
    assert X.judge_stream(adler, m) == XE_DATA
    cases.append(("adler", base(stream={1: adler}).fails(XE_DATA, 1)))
    cases.append(("dataSize above n", base(chunk_hdr={0: dict(size=n + 1)}).fails(XE_CHUNK, 0)))
    left, right = Exr(8, 35, RGBA, ZIP, seed=31), craft(33, 5, MIXED, tile=(16, 4), seed=32)
    for name, p in cases:
        try:
            X.run(t.reader, [left, p, right], align=16)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    # a forged record: compression 5 with one line a chunk
    files = [left, good, right]
    b = t.reader.headers(files)
    rec = b.rec.copy()
    rec[1]["lines_per_chunk"] = 1
    X._forged(t.reader, b, files, rec, b.chans, "lines_per_chunk")
    return len(cases) + 1


def mix():
    flagged = [p for name, p in X.header_faults() if name == "compression 4"][0]
    return [Exr(21, 40, RGBA, ZIP, seed=1), craft(21, 40, MIXED, seed=2, noise=(1,)), Exr(9, 7, MIXED, NONE, seed=3), flagged,
            Exr(33, 9, MIXED, ZIPS, seed=4), craft(40, 33, ONE_FLOAT, tile=(16, 16), order=2, seed=5), craft(300, 3, RGBA, seed=6)]


def read_independence(t):
    """ZIP, PXR24, NONE, a flagged compression-4 file and ZIPS in one call, in two slot orders and with duplicates; the same words and
    bytes at input alignments 0 .. 3; every file alone (n_files 1) against the batch"""
    files = mix()
    b0 = t.reader.headers(files)
    X.check_records(b0)
    ref = t.reader.read(b0, align=16)
    X.check_read(ref, files)
    n = 1
    for shift in (1, 2, 3):
        b = t.reader.headers(files, shift=shift, gap=shift)
        r = t.reader.read(b, align=16)
        assert (r.off, r.len, r.status, r.detail, r.out) == (ref.off, ref.len, ref.status, ref.detail, ref.out), shift
        n += 1
    for order in (list(range(len(files)))[::-1], [5, 1, 1, 0, 6, 3, 5, 2, 4, 1]):
        r = t.reader.read(b0, sel=order, align=16)
        X.check_read(r, files, sel=order)
        for j, k in enumerate(order):
            assert r.slot(j) == ref.slot(k)
        n += 1
    for k, p in enumerate(files):
        if p.flag:
            continue
        alone = t.reader.read(t.reader.headers([p]))
        assert alone.status == [0] and alone.slot(0) == p.want == ref.slot(k), k
        n += 1
    return n


# ---- writing ----------------------------------------------------------------------------------------------------------------------------------
def expected(t, p, pb, level, strategy):
    """the whole expected file: every chunk's stream is the zlib header + the payload of zmi_deflate_pieces_dev on the forward bytes
    alone + Adler-32 from zlib, or the raw bytes where that is not shorter than n"""
    st = {}
    for k, (raw, (x0, y0, w, h)) in enumerate(zip(p.raw, p.boxes)):
        d = forward(raw, w, h, p.channels)
        cand = zlib_header(level, strategy) + t.pw.payload(d, pb, level, strategy) + struct.pack(">I", zlib.adler32(d))
        if len(cand) < len(raw):
            st[k] = cand
    return Exr(p.width, p.height, p.channels, PXR24, xmin=p.xmin, ymin=p.ymin, tile=p.tile, planes=p.planes, display=p.display, stream=st,
               reference=False)


def write_check(t, r, files, pb=4096, level=6, strategy=0, align=1, exact=None, exact_files=None, exact_chunks=None):
    """every judge on a call that had room for all its files -> the chunks stored raw, per file"""
    assert r.rc == 0 and r.guard_ok, (r.rc, r.guard_ok, t.L.zmi_last_error())
    n, p0 = len(files), files[0]
    assert r.status == [0] * n, r.status
    assert r.off == expected_offsets(r.len, align), (r.off[:8], r.len[:8])
    assert r.off[n] <= t.bound(p0, n, pb=pb, level=level, strategy=strategy, align=align)
    exact = level in EXACT if exact is None else exact
    stored, regions = [], []
    for i, p in enumerate(files):
        blob = r.file(i)
        region, raw = read_file(blob, p)                                          # the reference reader
        assert region == lossy_region(p, raw), i
        assert [s for s, _ in W.chunks(blob, p)] == [int(x) for x in r.chunk_len[i]], i
        stored.append(raw)
        regions.append(region)
        if exact and (exact_files is None or i < exact_files) and (exact_chunks is None or p.n_chunks <= exact_chunks):
            want = expected(t, p, pb, level, strategy)
            assert raw == want.stored, (i, raw, want.stored)
            if blob != want.blob:
                bad = next(k for k in range(min(len(blob), len(want.blob))) if blob[k] != want.blob[k]) if len(blob) == len(want.blob) else -1
                raise AssertionError("file %d (%d x %d, %s, level %d): %d bytes, expected %d, first difference at %d"
                                     % (i, p.width, p.height, p.channels, level, len(blob), len(want.blob), bad))
    # the round trip on the device: the headers of the written batch are d_written, the read gives the reference reader's regions
    nch = len(p0.channels)
    b = t.reader.headers([types.SimpleNamespace(blob=r.file(i)) for i in range(n)], shift=3, gap=5, chan_cap=nch)
    assert b.rc == 0 and [int(x) for x in b.rec["status"]] == [0] * n
    assert [int(x) for x in b.rec["compression"]] == [PXR24] * n and [int(x) for x in b.rec["lines_per_chunk"]] == [16] * n
    assert b.rec.tobytes() == r.written.tobytes() and b.chans.tobytes() == r.wch.tobytes()
    rd = t.reader.read(b, align=4)
    assert rd.rc == 0 and rd.clean and rd.status == [0] * n and rd.detail == [0] * n, (rd.status, rd.detail)
    assert [rd.slot(j) for j in range(n)] == regions
    return stored


def write_run(t, files, **kw):
    wkw = {k: kw[k] for k in ("pb", "level", "strategy", "align", "shift") if k in kw}
    r = t.write([source(p) for p in files], **wkw)
    ckw = {k: kw[k] for k in ("pb", "level", "strategy", "align", "exact", "exact_files", "exact_chunks") if k in kw}
    r.stored = write_check(t, r, files, **ckw)
    return r


def write_geometry(t, widths=None, heights=(1, 15, 16, 17, 33), layouts=LAYOUTS):
    """every width x height x layout, two images a call; the expected file byte for byte on the first image of files of at most 2 chunks"""
    n = 0
    for li, layout in enumerate(layouts):
        for h in heights:
            for w in (widths or widths_of(t)):
                write_run(t, [craft(w, h, layout, seed=w + 3 * h + li + 7 * k, xmin=-(w % 3), ymin=-(h % 5)) for k in range(2)], align=16, shift=li,
                          pb=1024, exact_files=1, exact_chunks=2)
                n += 1
    return n


def write_tiles(t, sizes=((16, 16), (32, 8))):
    n = 0
    for tw, th in sizes:
        write_run(t, [craft(37, 21, MIXED, tile=(tw, th), seed=tw + k, xmin=-5, ymin=-3) for k in range(2)], align=16, pb=512)
        write_run(t, [craft(tw, th, RGBA, tile=(tw, th), seed=th, xmin=7, ymin=-9)], pb=512)
        n += 2
    return n


def write_values(t):
    T, n = t.p24_trip, 0
    for li, layout in enumerate(LAYOUTS):
        w, h = 2 * T + 3, 5
        write_run(t, [craft(w, h, layout, planes=[palette(ty, w, h, 7 * li + c) for c, (_, ty) in enumerate(layout)], seed=li)])
        write_run(t, [craft(T + 1, 2, layout, planes=[all_ff(ty, T + 1, 2) for _, ty in layout], seed=li)])
        n += 2
    r = write_run(t, [craft(T + 7, 3, ONE_FLOAT, planes=[special_floats(T + 7, 3, 5)], seed=1)])
    assert r.stored == [[False]]
    return n + 1


def write_raw_rule(t):
    """noise chunks among smooth ones: dataSize == n exactly at the noise chunks; level 0 on HALF channels (m = n): every chunk raw; a
    file of noise only"""
    a = [craft(70, 50, RGBA, noise=(1, 3), seed=3), craft(70, 50, RGBA, noise=(0,), seed=4)]
    assert write_run(t, a, pb=1024).stored == [[False, True, False, True], [True, False, False, False]]
    b = [craft(37, 21, ONE_HALF, tile=(16, 16), noise=(2, 5), seed=5)]
    assert write_run(t, b, pb=256).stored == [[False, False, True, False, False, True]]
    c = [craft(33, 20, RGBA, seed=6)]
    assert write_run(t, c, level=0).stored == [[True, True]]
    e = [craft(19, 20, RGBA, noise=(0, 1), seed=8)]
    assert write_run(t, e).stored == [[True, True]]
    return 4


def write_pieces(t, levels=(1, 6, 9, 0), set_group=None):
    """piece_bytes 256 and 1 MiB, 1 and 3 images a call, on chunks of several pieces (16 x 150 MIXED: m = 21 600 bytes); the same bytes
    in one launch group and in forced groups of one chunk"""
    files, n = [craft(150, 20, MIXED, seed=9), craft(150, 20, MIXED, noise=(1,), seed=10), craft(150, 20, MIXED, seed=11)], 0
    for level in levels:
        for pb in (256, 1 << 20):
            for count in (1, 3):
                write_run(t, files[:count], pb=pb, level=level, align=16)
                n += 1
    if set_group:
        src = [source(p) for p in files]
        ref = t.write(src, pb=256, align=16)
        for g in (85, 100):
            set_group(g)
            try:
                r = t.write(src, pb=256, align=16)
            finally:
                set_group(None)
            assert (r.rc, r.off, r.len, r.status, r.out) == (0, ref.off, ref.len, ref.status, ref.out), g
            assert r.chunk_len.tobytes() == ref.chunk_len.tobytes() and r.guard_ok
            n += 1
    return n


def write_independence(t, shifts=(0, 1, 2, 3)):
    p = craft(61, 35, MIXED, noise=(1,), seed=14)
    others = [craft(61, 35, MIXED, seed=15 + k) for k in range(3)]
    ref, n = write_run(t, [p]).file(0), 0
    for shift in shifts:
        assert t.write([source(p)], shift=shift).file(0) == ref
        n += 1
    r = t.write([source(x) for x in others[:2] + [p] + others[2:]], align=16)
    assert r.rc == 0 and r.guard_ok and r.status == [0] * 4 and r.file(2) == ref
    return n + 1
