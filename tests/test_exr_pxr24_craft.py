"""The judges of tests/exr_pxr24_checks.py against the byte-exact examples of the format's description (include/zmi355.h, OpenEXR
PXR24) and against each other: no library, no GPU."""
import zlib

import numpy as np

import exr_pxr24_checks as K
from exr_checks import HALF, FLOAT, UINT, MIXED, RGBA, ONE_HALF

EXAMPLE = (("G", HALF), ("Z", FLOAT), ("id", UINT))
RAW = bytes.fromhex("003c 0040 0042 0000003f 0000c0bf 00002040 07000000 05000000 04030201")
INFLATED = bytes.fromhex("3c 04 02 00 00 00  3f 80 80 00 c0 60 00 00 00  00 ff 01 00 ff 02 00 ff 02 07 fe ff")
F24 = [(0x3F000000, 0x3F0000), (0x3F8000FF, 0x3F8001), (0x3F80007F, 0x3F8000), (0x3F800080, 0x3F8001), (0x7F7FFFFF, 0x7F7FFF),
       (0x7F800000, 0x7F8000), (0x7F800001, 0x7F8001), (0xFFC12345, 0xFFC123), (0x80000000, 0x800000), (0x000000FF, 0x000001),
       (0xBFC00000, 0xBFC000)]


def test_the_example_in_both_directions():
    assert len(RAW) == 30 and len(INFLATED) == 27
    assert K.pxr24_forward(RAW, 3, 1, EXAMPLE) == INFLATED
    assert K.pxr24_forward_fast(RAW, 3, 1, EXAMPLE) == INFLATED
    assert K.pxr24_undo(INFLATED, 3, 1, EXAMPLE) == RAW                   # (0.5, -1.5 and 2.5 fit 24 bits)
    assert len(zlib.compress(INFLATED, 6)) == 33                          # ... so in a real file this chunk is stored raw
    p = K.craft(3, 1, EXAMPLE, planes=[np.frombuffer(RAW[:6], "<f2").reshape(1, 3), np.frombuffer(RAW[6:18], "<f4").reshape(1, 3),
                                       np.frombuffer(RAW[18:], "<u4").reshape(1, 3)])
    assert p.raw == [RAW] and p.stored == [True] and p.want == RAW[:6] + bytes([K.FILL]) * 2 + RAW[6:]   # (the Z plane at a multiple of 4)


def test_f24_table():
    for u, want in F24:
        assert K.f24(u) == want, hex(u)
    assert K.f24_fast(np.array([u for u, _ in F24], dtype=np.uint32)).tolist() == [w for _, w in F24]


def test_f24_vectorised_against_the_loop():
    rng = np.random.RandomState(1)
    bits = [int(x) for x in rng.randint(0, 1 << 32, 1 << 16, dtype=np.int64)]
    for se in range(512):
        for m in (0, 1, 0x7F, 0x80, 0xFF, 0x7FFF80, 0x7FFFFF):
            bits.append(se << 23 | m)
    got = K.f24_fast(np.array(bits, dtype=np.uint32))
    want = np.array([K.f24(u) for u in bits], dtype=np.uint32)
    assert np.array_equal(got, want)
    # a NaN stays a NaN, an infinity an infinity, and rounding never makes one
    b = np.array(bits, dtype=np.int64)
    e, m = b & 0x7F800000, b & 0x7FFFFF
    g = got.astype(np.int64)
    is_nan, is_inf = (e == 0x7F800000) & (m != 0), (e == 0x7F800000) & (m == 0)
    assert np.array_equal((g & 0x7F8000) == 0x7F8000, is_nan | is_inf) and np.array_equal(((g & 0x7F8000) == 0x7F8000) & ((g & 0x7FFF) != 0), is_nan)


def test_forward_against_undo_over_the_geometry():
    """every width x height x layout on ramps, random words and the special floats: both forwards agree, and the undo gives the pixels
    with f24 << 8 in the FLOAT planes"""
    n = 0
    for li, layout in enumerate(K.LAYOUTS):
        for h in (1, 15, 16, 17):
            for w in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 513):
                for kind in range(3):
                    if kind == 0:
                        planes = [K.ramp(t, w, h, li + c) for c, (_, t) in enumerate(layout)]
                    elif kind == 1:
                        planes = [K.palette(t, w, h, w + c, k=64) for c, (_, t) in enumerate(layout)]
                    else:
                        planes = [K.special_floats(w, h, w) if t == FLOAT else K.all_ff(t, w, h) for _, t in layout]
                    raw = np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(h, -1) for p in planes], axis=1).tobytes()
                    d = K.pxr24_forward_fast(raw, w, h, layout)
                    if w * h <= 1024:
                        assert d == K.pxr24_forward(raw, w, h, layout), (layout, w, h, kind)
                    lossy = [K.f24_fast(p.view("<u4")) << np.uint32(8) if t == FLOAT else p for p, (_, t) in zip(planes, layout)]
                    want = np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(h, -1) for p in lossy], axis=1).tobytes()
                    assert K.pxr24_undo(d, w, h, layout) == want, (layout, w, h, kind)
                    n += 1
    assert n == 5 * 4 * 11 * 3


def test_the_crafter_and_the_file_reader():
    """a crafted file with compressed and raw-stored chunks, scanlines and tiles: the reference reader returns the wanted region"""
    for p in (K.craft(70, 50, MIXED, noise=(1,), seed=3), K.craft(37, 21, RGBA, tile=(16, 16), order=0, noise=(2,), seed=4),
              K.craft(5, 3, ONE_HALF, seed=5)):
        region, stored = K.read_file(p.blob, p)
        assert stored == p.stored and region == p.want
    p = K.craft(70, 50, MIXED, seed=3)
    assert not any(p.stored) and p.want != p.source and len(p.want) == len(p.source) == p.region_bytes
