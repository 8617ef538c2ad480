"""CPU tests, no library: the judges of tests/tiff_write_checks.py against each other, against tiff_checks' crafter and reference
predictors, and against PIL with libtiff in both directions (PIL reads what craft() makes; parse() reads what PIL writes)."""
import io

import numpy as np
import pytest

import tiff_checks as TC
import tiff_write_checks as K

PIL_CASES = [K.Case(37, 21, 1, 8, 1, 2, rps=8, seed=1), K.Case(37, 21, 3, 8, 1, 2, tile=(16, 16), seed=2),
             K.Case(37, 21, 4, 8, 1, 2, rps=5, extra=1, seed=3), K.Case(37, 21, 1, 16, 1, 2, tile=(16, 32), seed=4),
             K.Case(37, 21, 1, 32, 3, 3, rps=8, seed=5), K.Case(21, 37, 1, 32, 3, 3, tile=(16, 16), big=True, seed=6),
             K.Case(5, 3, 3, 8, 1, 1, seed=7), K.Case(33, 9, 3, 8, 1, 2, rps=2, big=True, seed=8)]


def test_pil_has_libtiff():
    """judge (c) must run on this project's machines, not skip"""
    assert K.HAVE_PIL


@pytest.mark.parametrize("k", range(len(PIL_CASES)))
def test_pil_reads_the_crafted_file(k):
    c = PIL_CASES[k]
    assert K.pil_reads(c)
    for align in (1, 16):
        f = K.craft(c, K.host_streams(c, c.segs_zero), align)
        assert K.pil_pixels(f) == c.image


def test_crafter_against_parser():
    """every depth, sample count and predictor, classic and BigTIFF, strips and tiles: parse(craft(x)) gives x and the tags of *w"""
    n = 0
    for k, (bits, samples, pred, fmt) in enumerate(K.format_cases()):
        c = K.Case(21, 19, samples, bits, fmt, pred, tile=(16, 16) if k & 2 else None, rps=None if k & 2 else 5, big=bool(k & 1),
                   extra=1 if samples in (2, 4) else 0, seed=k)
        for align in (1, 2, 4096):
            f = K.craft(c, K.host_streams(c, c.segs), align)
            tags, segs = K.parse(f)
            K.check_tags(tags, c, align)
            assert segs == c.segs
        n += 1
    assert n == 44 + 7


def test_layout_rules():
    """the fixed bytes the header states, on a file small enough to read: the header, the entry count, the inline arrays of a
    one-segment page, the even positions of the out-of-line values, zero gaps"""
    c = K.Case(5, 3, 3, 8, 1, 2, seed=1)
    f = K.craft(c, [b"SEGMENT"], 16)
    assert f[:8] == bytes.fromhex("49492A0008000000") and f[8:10] == (12).to_bytes(2, "little")
    tags = {int.from_bytes(f[10 + 12 * q:12 + 12 * q], "little"): f[10 + 12 * q:22 + 12 * q] for q in range(12)}
    assert sorted(tags) == [256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 339]
    at = 10 + 12 * 12 + 4                                                    # 258 and 339: 6 bytes each, out of line
    assert tags[258][8:] == at.to_bytes(4, "little") and tags[339][8:] == (at + 6).to_bytes(4, "little")
    seg = -(-(at + 12) // 16) * 16
    assert tags[273][2:] == b"\x04\0\x01\0\0\0" + seg.to_bytes(4, "little") and tags[279][8:] == (7).to_bytes(4, "little")
    assert tags[317][2:] == b"\x03\0\x01\0\0\0\x02\0\0\0" and f[10 + 144:at] == bytes(4)
    assert f[at + 12:seg] == bytes(seg - at - 12) and f[seg:] == b"SEGMENT"
    b = K.Case(5, 3, 3, 8, 1, 2, seed=1, big=True)
    f = K.craft(b, [b"SEGMENT"], 1)
    assert f[:16] == bytes.fromhex("49492B0008000000") + (16).to_bytes(8, "little") and f[16:24] == (12).to_bytes(8, "little")
    assert len(f) == 16 + 8 + 12 * 20 + 8 + 7                               # three SHORTs fit the 8-byte value field: nothing out of line


def test_parser_against_the_reader_tests_crafter():
    """tiff_checks.Tiff is written on its own (segments first, the IFD last, PIL-pinned by tests/test_tiff_craft.py): parse() reads it"""
    n = 0
    for big in (False, True):
        for arrays in (TC.LONG, TC.LONG8):
            for p in (TC.Page(37, 21, 3, 8, pred=2, tile=(16, 16), arrays=arrays, seed=1), TC.Page(20, 9, 1, 32, 3, 3, rps=4, arrays=arrays, seed=2),
                      TC.Page(9, 7, 2, 16, 2, 1, rps=3, arrays=arrays, seed=3)):
                tags, segs = K.parse(TC.Tiff([p], big=big).blob, strict=False)
                assert segs == p.segs and tags[256][1] == [p.width]
                n += 1
    assert n == 12


@pytest.mark.skipif(not K.HAVE_PIL, reason="PIL with libtiff")
def test_parser_reads_what_pil_writes():
    rs = np.random.RandomState(3)
    for mode, dtype, shape in (("L", np.uint8, (21, 37)), ("RGB", np.uint8, (21, 37, 3)), ("I;16", np.uint16, (21, 37)), ("F", np.float32, (21, 37))):
        a = rs.randint(0, 256, int(np.prod(shape)) * np.dtype(dtype).itemsize).astype(np.uint8).view(dtype).reshape(shape)
        if dtype == np.float32:
            a = np.nan_to_num(a, nan=1.0)
        buf = io.BytesIO()
        im = K.Image.fromarray(a)
        assert im.mode == mode
        im.save(buf, format="TIFF", compression="tiff_adobe_deflate")
        tags, segs = K.parse(buf.getvalue(), strict=False)
        assert b"".join(segs) == a.astype(a.dtype.newbyteorder("<")).tobytes()


def test_predict_is_the_inverse_of_unpredict():
    for bits, samples, pred, fmt in K.format_cases():
        c = K.Case(19, 5, samples, bits, fmt, pred, seed=bits + samples)
        raw = c.predicted(c.segs, 0)                                         # (asserts the round trip)
        assert (raw == c.segs[0]) == (pred == 1)
