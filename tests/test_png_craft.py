"""The two judges of tests/png_checks.py -- the crafter with its forward filters, and the reference unfilter -- pinned: against each
other by a round trip everywhere, and against PIL (its decoder reads the crafter's files; the reference unfilter reads the files its
encoder writes) where PIL can be imported."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_checks as K


def test_round_trip_of_filters_and_reference():
    """every filter type on every row, and mixed, at every bpp: unfilter(filter_rows(x)) == x, and a None row is the bytes themselves"""
    for colour, depth in K.FORMATS:
        for types in ([0] * 6, [1] * 6, [2] * 6, [3] * 6, [4] * 6, [4, 3, 2, 1, 0, 4], K.adaptive(6, depth)):
            p = K.Png(7, 6, colour, depth, types, seed=colour + depth)
            assert K.unfilter(p.scan, 6, p.row_bytes, p.bpp) == p.raw
            if types[0] == 0:
                assert p.scan[1:1 + p.row_bytes] == p.raw[:p.row_bytes]
    assert K.unfilter(bytes([5, 1, 2]), 1, 2, 1) is None


def test_filter_cases_hold_what_they_name():
    """the tie and wrap cases of the filter matrix produce the situations they are there for"""
    raw = bytes(50 if (r + i) % 2 else 40 for r in range(5) for i in range(6))
    a, b, c = raw[6 + 0], raw[1], raw[0]                                  # row 1, column 1
    assert a == b != c and abs(b - c) == abs(a - c) < abs(a + b - 2 * c) and K.paeth(a, b, c) == a
    raw = bytes(100 + 40 * i - 20 * r for r in range(4) for i in range(4))
    a, b, c = raw[4], raw[1], raw[0]
    assert abs(a - c) == abs(a + b - 2 * c) < abs(b - c) and K.paeth(a, b, c) == b
    assert K.paeth(90, 90, 90) == 90
    avg = K.Png(8, 4, 0, 8, 3, raw=bytes([255]) * 32)
    assert avg.scan[9 + 2] == 0                                            # 255 - ((255 + 255) >> 1): a sum kept in 8 bits would give 128
    sub = K.Png(8, 3, 0, 8, 1, raw=bytes((i * 200) & 0xFF for i in range(24)))
    assert any(sub.raw[i] < sub.raw[i - 1] for i in range(1, 8))          # a difference that wraps


def test_chunks_and_split():
    p = K.Png(30, 20, 6, 8, K.adaptive(20), seed=8, split=[1, 0, 3])
    at, got, n = 8, b"", 0
    while at < len(p.blob):
        ln, ct = struct.unpack(">I4s", p.blob[at:at + 8])
        assert zlib.crc32(p.blob[at + 4:at + 8 + ln]) == struct.unpack(">I", p.blob[at + 8 + ln:at + 12 + ln])[0]
        if ct == b"IDAT":
            if n == 0:
                assert at == p.idat_pos
            assert ln == ([1, 0, 3] + [len(p.stream) - 4])[n]
            got += p.blob[at + 8:at + 8 + ln]
            n += 1
        at += 12 + ln
    assert n == p.n_idat == 4 and got == p.stream and zlib.decompress(got) == p.scan and len(got) == p.idat_bytes


def test_crafter_against_pil():
    """PIL decodes the crafter's files to the crafter's bytes: five filters, colour types 0, 2, 4 and 6 at depth 8, gray at 16 bits,
    palette at 8 bits, with the IDAT split 1 / 0 / 3 / rest"""
    Image = pytest.importorskip("PIL.Image")
    for colour, depth, mode in ((0, 8, "L"), (2, 8, "RGB"), (4, 8, "LA"), (6, 8, "RGBA"), (0, 16, "I;16"), (3, 8, "P")):
        for types in (0, 1, 2, 3, 4, K.adaptive(11, colour)):
            p = K.Png(9, 11, colour, depth, types, seed=colour + depth, split=[1, 0, 3])
            im = Image.open(io.BytesIO(p.blob))
            im.load()
            assert im.size == (9, 11) and im.mode in (mode, "I;16B"), (im.mode, mode)
            got = im.tobytes()
            want = p.raw if im.mode != "I;16" else K.swap16(p.raw)
            assert got == want, (colour, depth, types)
    p = K.Png(9, 11, 2, 8, K.adaptive(11), seed=4, junk=b"junk behind the stream")
    im = Image.open(io.BytesIO(p.blob))
    im.load()
    assert im.tobytes() == p.raw                                          # bytes behind the zlib stream inside IDAT: accepted


def test_reference_unfilter_against_pil_encoder():
    """PIL writes a PNG (its encoder picks the filters); the reference unfilter gives back the pixels"""
    Image = pytest.importorskip("PIL.Image")
    rnd = np.random.RandomState(5)
    for mode, ch in (("L", 1), ("RGB", 3), ("RGBA", 4)):
        arr = (np.cumsum(rnd.randint(-3, 4, (37, 41, ch)), axis=1) & 0xFF).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr.squeeze() if ch == 1 else arr, mode).save(buf, "PNG")
        blob = buf.getvalue()
        at, idat = 8, b""
        while at < len(blob):
            ln, ct = struct.unpack(">I4s", blob[at:at + 8])
            if ct == b"IDAT":
                idat += blob[at + 8:at + 8 + ln]
            at += 12 + ln
        scan = zlib.decompress(idat)
        assert K.unfilter(scan, 37, 41 * ch, ch) == arr.tobytes()
