"""The judges of the OpenEXR writer's tests, judged (CPU, no library): the crafter of tests/exr_checks.py with injected streams -- what
exr_write_checks.Target.expected builds the expected file from -- against the reference reader, the injected-stream rule against
test_exr_craft's own pin of the store-raw rule, and the chunk parser of tests/exr_write_checks.py against the crafter's layout."""
import struct
import zlib

import numpy as np

import exr_checks as X
import exr_write_checks as K
from test_exr_craft import PIN2, PIN2_G, PIN2_Z


def _streams(p, level, compress=zlib.compress):
    """the rule of judge (b), with zlib standing in for the device encoder"""
    out = {}
    for k, raw in enumerate(p.raw):
        cand = compress(X.zip_forward(raw), level)
        out[k] = cand if len(cand) < len(raw) else raw
    return out


def test_injected_streams_are_read_by_the_reference():
    """a file whose every stream is injected -- another level, and a stream cut into two deflate pieces as the device encoder cuts it --
    reads as the same pixels; Exr.__init__ runs read_exr on it and compares the planes"""
    def two_pieces(d, level):
        c = zlib.compressobj(level)
        half = len(d) // 2
        return c.compress(d[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(d[half:]) + c.flush()

    n = 0
    for layout in X.LAYOUTS:
        for comp, tile in ((X.ZIP, None), (X.ZIPS, None), (X.ZIP, (16, 16))):
            p = X.Exr(37, 21, layout, comp, tile=tile, xmin=-5, ymin=3, seed=n)
            for level, fn in ((1, zlib.compress), (9, two_pieces)):
                q = X.Exr(37, 21, layout, comp, tile=tile, xmin=-5, ymin=3, planes=p.planes, stream=_streams(p, level, fn))
                assert q.want == p.want and q.table_pos == p.table_pos and [len(r) for r in q.raw] == [len(r) for r in p.raw]
                assert q.stored == [len(q.data[k]) == len(p.raw[k]) for k in range(p.n_chunks)]
                n += 1
    assert n == 18


def test_the_injected_stream_rule_is_the_crafters_own():
    """with zlib at the crafter's level the injected streams are exactly the crafter's data: the rule `raw where the candidate is not
    shorter` is the one test_exr_craft pins, both outcomes included"""
    outcomes = set()
    for comp in (X.ZIPS, X.ZIP):
        p = X.Exr(3, 2, (("G", X.HALF), ("Z", X.FLOAT)), comp, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z])
        s = _streams(p, 6)
        assert [s[k] for k in range(p.n_chunks)] == p.data
        assert X.Exr(3, 2, (("G", X.HALF), ("Z", X.FLOAT)), comp, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z], stream=s).blob == p.blob
    for p in (X.Exr(70, 50, X.RGBA, X.ZIP, noise=(1, 3), seed=3), X.Exr(1, 3, X.ONE_HALF, X.ZIPS, seed=7)):
        s = _streams(p, 6)
        assert [s[k] for k in range(p.n_chunks)] == p.data
        outcomes |= set(p.stored)
    assert outcomes == {True, False}
    assert len(X.Exr(1, 3, X.ONE_HALF, X.ZIPS, seed=7).raw[0]) == 2


def test_the_chunk_parser_against_the_crafter():
    for p in (X.Exr(37, 21, X.RGBA, X.ZIP, tile=(16, 16), noise=(2,), xmin=-5, ymin=3, seed=1), X.Exr(33, 40, X.MIXED, X.ZIP, noise=(1,), ymin=-7, seed=2),
              X.Exr(9, 5, X.ONE_HALF, X.NONE, seed=3)):
        got = K.chunks(p.blob, p)
        assert [d for _, d in got] == p.data and [s for s, _ in got] == [len(d) for d in p.data]
    p = X.Exr(3, 2, (("G", X.HALF), ("Z", X.FLOAT)), X.NONE, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z])
    assert [d for _, d in K.chunks(PIN2, p)] == p.raw
    # a gap in front of a chunk, a wrong y and a shuffled physical order are all refused
    for q in (X.Exr(9, 5, X.ONE_HALF, X.NONE, seed=3, chunk_hdr={2: dict(y=7)}, reference=False),
              X.Exr(9, 40, X.ONE_HALF, X.ZIP, seed=3, order=1)):
        try:
            K.chunks(q.blob, q)
        except AssertionError:
            continue
        raise AssertionError("the parser took a file no writer of this library may write")


def test_the_description_of_a_layout():
    """the ctypes mirror of zmi_exr_write: sizes and the fields describe() fills"""
    p = X.Exr(37, 21, X.MIXED, X.ZIP, tile=(16, 8), xmin=-5, ymin=3, display=(0, 0, 99, 49), seed=1)
    w, keep = K.describe(p, pb=512, level=9, strategy=2, align=64)
    assert tuple(w.data_window) == (-5, 3, 31, 23) and tuple(w.display_window) == (0, 0, 99, 49) and w.n_channels == 3
    assert [(w.channels[c].name, w.channels[c].pixel_type) for c in range(3)] == [(b"G", X.HALF), (b"Z", X.FLOAT), (b"id", X.UINT)]
    assert (w.compression, w.tile_w, w.tile_h, w.flags, w.piece_bytes, w.out_align, w.level, w.strategy) == (3, 16, 8, 0, 512, 64, 9, 2)
    assert struct.calcsize("8iI4xP6I2i") == K.C.sizeof(K.Write) and np.dtype(X.IMAGE).itemsize == 88
