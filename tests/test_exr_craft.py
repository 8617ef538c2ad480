"""The judges of the OpenEXR tests, judged (CPU, no library): the crafter and the reference reader of tests/exr_checks.py against the two
byte-exact examples the format's description carries (include/zmi355.h), and against each other over the matrices the device tests use.
No OpenEXR library exists where these tests run, so these pins are all that stands behind the judges."""
import struct
import zlib

import numpy as np

import exr_checks as K

PIN1_D = bytes.fromhex("00808080e619bd8482826a")
PIN1_RAW = bytes.fromhex("003c004000420044662eff")
PIN2 = bytes.fromhex(
    "762f3101020000006368616e6e656c730063686c69737400250000004700010000000000000001000000010000005a0002000000000000000100000001000000"
    "00636f6d7072657373696f6e00636f6d7072657373696f6e0001000000006461746157696e646f7700626f7832690010000000ffffffff05000000010000000600"
    "0000646973706c617957696e646f7700626f7832690010000000000000000000000002000000010000006c696e654f72646572006c696e654f7264657200010000"
    "0000706978656c417370656374526174696f00666c6f617400040000000000803f73637265656e57696e646f7743656e7465720076326600080000000000000000"
    "00000073637265656e57696e646f77576964746800666c6f617400040000000000803f0037010000000000005101000000000000050000001200000000"
    "3c004000420000003f0000c03f00002040060000001200000000440045004600006040000090400000b040")
PIN2_G = np.array([[1, 2, 3], [4, 5, 6]], dtype="<f2")
PIN2_Z = np.array([[.5, 1.5, 2.5], [3.5, 4.5, 5.5]], dtype="<f4")


def test_pin_1_the_predictor_and_the_interleave():
    assert K.unzip(PIN1_D) == PIN1_RAW
    assert K.zip_forward(PIN1_RAW) == PIN1_D and K.zip_forward_fast(PIN1_RAW) == PIN1_D
    # by hand: t[i] = t[i - 1] + d[i] - 128, then the two halves alternate
    t = [PIN1_D[0]]
    for x in PIN1_D[1:]:
        t.append((t[-1] + x - 128) % 256)
    assert bytes(t) == bytes.fromhex("0000000066ff3c404244" + "2e")
    assert bytes(t[i // 2] if i % 2 == 0 else t[6 + i // 2] for i in range(11)) == PIN1_RAW


def test_pin_2_the_crafter_writes_it_byte_for_byte():
    assert len(PIN2) == 363
    p = K.Exr(3, 2, (("G", K.HALF), ("Z", K.FLOAT)), K.NONE, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z])
    assert p.table_pos == 295 and struct.unpack_from("<2Q", p.blob, 295) == (311, 337)
    assert p.blob == PIN2


def test_pin_2_the_reference_reads_it():
    r = K.read_exr(PIN2)
    assert r["channels"] == [("G", K.HALF), ("Z", K.FLOAT)] and r["data_window"] == (-1, 5, 1, 6) and r["display_window"] == (0, 0, 2, 1)
    assert not r["tiled"] and r["planes"][0].tolist() == PIN2_G.tolist() and r["planes"][1].tolist() == PIN2_Z.tolist()
    assert r["region"] == PIN2_G.tobytes() + PIN2_Z.tobytes() and len(r["region"]) == 12 + 24


def test_pin_2_compressed_round_trip():
    """the same pixels under ZIPS and ZIP: chunks of 18 and 36 bytes do not shrink much, so pin both outcomes of the store-raw rule"""
    for comp in (K.ZIPS, K.ZIP):
        p = K.Exr(3, 2, (("G", K.HALF), ("Z", K.FLOAT)), comp, xmin=-1, ymin=5, planes=[PIN2_G, PIN2_Z])
        for raw, data, stored in zip(p.raw, p.data, p.stored):
            packed = zlib.compress(K.zip_forward(raw), 6)
            assert stored == (len(packed) >= len(raw)) and data == (raw if stored else packed)
        assert p.want == PIN2_G.tobytes() + PIN2_Z.tobytes()


def test_forward_transforms_agree_and_invert():
    rng = np.random.RandomState(5)
    for n in (1, 2, 3, 4, 5, 11, 64, 255, 1000, 4097):
        raw = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        d = K.zip_forward(raw)
        assert K.zip_forward_fast(raw) == d and K.unzip(d) == raw, n
    assert K.unzip(bytes([255] * 700)) == bytes((255 * (i // 2 + 1 + (350 if i % 2 else 0)) - 128 * (i // 2 + (350 if i % 2 else 0))) % 256
                                                  for i in range(700))


def test_crafter_against_reference_over_the_matrices():
    """every file the device tests craft is read back by the reference inside Exr.__init__ (pixels and layout); here the counts, the
    chunk geometry and the store-raw rule are pinned on top"""
    n = 0
    for layout in K.LAYOUTS:
        for comp in (K.ZIPS, K.ZIP, K.NONE):
            for h in (1, 15, 16, 17, 33):
                for w in (1, 2, 3, 5, 17, 63, 64, 65, 257):
                    p = K.Exr(w, h, layout, comp, seed=w + h)
                    assert p.n_chunks == -(-h // K.LINES[comp]) and sum(len(r) for r in p.raw) == h * p.row_bytes
                    assert all(s == (len(d) == len(r)) and len(d) <= len(r) for s, d, r in zip(p.stored, p.data, p.raw))
                    if comp == K.NONE:
                        assert all(p.stored)
                    n += 1
    assert n == 405
    p = K.Exr(37, 21, K.RGBA, K.ZIP, tile=(16, 16), order=2, seed=3)
    assert p.n_chunks == 6 and [b[2:] for b in p.boxes] == [(16, 16), (16, 16), (5, 16), (16, 5), (16, 5), (5, 5)] and p.phys != sorted(p.phys)
    assert K.Exr(40, 40, K.RGBA, K.ZIP, order=1).phys == [2, 1, 0]
    q = K.Exr(70, 50, K.RGBA, K.ZIP, noise=(1, 3), seed=3)
    assert q.stored == [False, True, False, True]


def test_the_fault_lists_hold_every_status():
    heads, chunks = K.header_faults(), K.chunk_faults()
    assert {p.flag for _, p in heads} == set(range(K.XE_MAGIC, K.XE_BIG + 1))
    assert {p.expect[1] & 0xFF for _, p in chunks} == {0, K.XE_CHUNK, K.XE_MISSING, K.XE_DATA, K.XE_LENGTH}
    assert len(heads) == 40 and len(chunks) == 26
    for name, p in chunks:                                                # a chunk fault leaves the header readable
        assert p.flag == 0, name
