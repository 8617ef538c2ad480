"""The judges of tests/png_write_checks.py against each other, on the CPU and without the library: the chooser on the constructed rows
(the GPU test cannot pass on inputs that never reach a branch), the crafter against the parser, PIL and zlib."""
import zlib

import pytest

import png_checks as P
import png_write_checks as K


def test_chooser_on_the_constructed_rows():
    """every type wins a row, the rows the docstring names tie exactly, and the winning row of the last one holds bytes of 0x80"""
    im = K.five_rows()
    types, costs = K.choose(im.raw, im.height, im.row_bytes, im.bpp)
    assert types == K.FIVE_TYPES and set(types) == {0, 1, 2, 3, 4}
    for r, (a, b) in K.FIVE_TIES.items():
        assert costs[r][a] == costs[r][b] == min(costs[r]) and types[r] == min(a, b), (r, costs[r])
    assert costs[0][0] == costs[0][2] and costs[0][1] == costs[0][4]          # row 0: the built-in ties
    for r, t in enumerate(types):                                             # everywhere else the winner stands alone
        others = [costs[r][k] for k in range(5) if k != t and (r not in K.FIVE_TIES or k not in K.FIVE_TIES[r])]
        assert min(others) > costs[r][t], (r, costs[r])
    scan = K.scanlines(im, K.ADAPTIVE)
    last = scan[6 * 33:]
    assert last[0] == 0 and last.count(0x80) == 8 and K.cost(last[1:]) == 8 * 128
    assert [scan[r * 33] for r in range(7)] == K.FIVE_TYPES


def test_cost_of_0x80_is_128_either_way():
    assert K.cost(bytes([0x80])) == 128 and K.cost(bytes([0x7F, 0x81, 0, 255, 1])) == 127 + 127 + 0 + 1 + 1


@pytest.mark.parametrize("args", [(2, 8), (6, 16, 5, 7), (0, 4, 13, 6)])
def test_stress_images_reach_every_branch(args):
    im = K.stress(*args)
    assert K.paeth_outcomes(im) == {"a", "b", "c", "tie", "carry"}
    for filt in range(6):
        scan = K.scanlines(im, filt)
        assert P.unfilter(scan, im.height, im.row_bytes, im.bpp) == im.raw
    types = K.choose(im.raw, im.height, im.row_bytes, im.bpp)[0]
    assert types[0] in (0, 1, 3)                                              # row 0: never Up or Paeth


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (3, 0), (6, 0), (9, 0), (-1, 0)])
def test_zlib_header_is_zlibs(level, strategy):
    assert K.zlib_header(level, strategy) == zlib.compress(b"abc", level)[:2]


def test_crafter_parser_and_pil_agree():
    """a crafted file around a zlib payload parses to its scanlines, and PIL reads the pixels of every format it keeps"""
    done = 0
    for colour, depth in K.FORMATS:
        if colour == 3:
            continue
        im = K.Img(7, 5, colour, depth, seed=depth)
        scan = K.scanlines(im, K.ADAPTIVE)
        payload = zlib.compress(scan, 6)[2:-4]
        f = K.craft(im, scan, payload, 6, 0)
        assert K.parse(f) == (7, 5, depth, colour, scan)
        if K.Image is not None and (depth == 8 or (depth == 16 and colour == 0)):
            assert K.pil_pixels(f) == im.raw
            done += 1
        assert P.Png(7, 5, colour, depth, types=K.choose(im.raw, 5, im.row_bytes, im.bpp)[0], raw=im.raw).scan == scan
    assert K.Image is None or done == 5


def test_parser_refuses_a_wrong_crc_and_a_second_idat():
    im = K.Img(3, 2, 2, 8)
    scan = K.scanlines(im, 0)
    f = K.craft(im, scan, zlib.compress(scan)[2:-4], 6, 0)
    K.parse(f)
    with pytest.raises(AssertionError):
        K.parse(f[:40] + bytes([f[40] ^ 1]) + f[41:])
    with pytest.raises(AssertionError):
        K.parse(f[:-12] + P.chunk(b"IDAT", b"") + f[-12:])


def test_expected_offsets():
    assert K.expected_offsets([5, 0, 17], 16) == [0, 16, 16, 48] and K.expected_offsets([5, 0, 17], 1) == [0, 5, 5, 22]
