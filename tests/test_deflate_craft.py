"""CPU tests of the crafter (tests/deflate_craft.py) and of the hand-built streams (tests/dynamic_block_checks.py): the table search
gives the capacities csrc/inflate.hip is built with, and the plain decoder inflate_ref -- the judge of the emulator and GPU tests
of these streams -- is held to the oracle (pinned on the reference), to system zlib and to the reference's own vectors."""
import json
import os
import random
import zlib

import pytest

import deflate_craft as D
import dynamic_block_checks as K
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_worst_tables_are_the_capacities_of_the_decode_kernel():
    """INF_LSIZE 852 (root 9, 286 symbols), INF_DSIZE 400 (root 8, 30 symbols), and zlib's published 592 for root 6 as the check
    of the search itself; the vectors come out of the search"""
    e9, c9 = D.worst_table(9, 286)
    e8, c8 = D.worst_table(8, 30)
    e6, c6 = D.worst_table(6, 30)
    assert (e9, e8, e6) == (852, 400, 592)
    rng = random.Random(1)
    for root, n, counts, want in ((9, 286, c9, 852), (8, 30, c8, 400), (6, 30, c6, 592)):
        assert sum(counts) == n and sum(c << (15 - l) for l, c in enumerate(counts, 1)) == 1 << 15
        for _ in range(3):
            assert D.table_size(D.from_counts(counts, rng), root) == want
    src = open(os.path.join(os.path.dirname(HERE), "zlib_rs_amd", "csrc", "inflate.hip")).read()
    assert "#define INF_LSIZE 852u" in src and "#define INF_DSIZE 400u" in src and "#define INF_LROOT 9u" in src and "#define INF_DROOT 8u" in src
    # no code of the random generators comes near them, which is why they have to be searched for
    assert max(D.table_size(D.random_complete(286, rng, True), 9) for _ in range(20)) < 852


def test_canonical_and_generators():
    assert D.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]          # the example of RFC 1951 section 3.2.2
    rng = random.Random(2)
    for n in (2, 30, 257, 286):
        for deep in (False, True):
            lens = D.random_complete(n, rng, deep)
            assert len(lens) == n and max(lens) <= 15 and sum(1 << (15 - l) for l in lens) == 1 << 15
    assert max(D.random_complete(286, rng, True)) == 15
    assert sorted(l for l in D.comb([5, 1, 9, 7], 12) if l) == [1, 2, 3, 3]


def test_inflate_ref_on_the_reference_vectors(o):
    """every raw bitstream of tests/golden/inflate_vectors.json: the oracle's status, and its bytes where that is 0"""
    vs = [v for v in json.load(open(os.path.join(HERE, "golden", "inflate_vectors.json")))["bitstreams"] if v["wrap"] == 0]
    assert len(vs) >= 10
    for v in vs:
        s = bytes.fromhex(v["input"])
        cap = 8 * len(s) + 64
        rc, out, used, msg = o.inflate(s, cap, 0)
        st, got, bits, kind = D.inflate_ref(s, cap)
        assert st == (0 if rc == 1 else rc), (v["source"], st, rc, kind, msg)
        assert K.MESSAGE.get(kind) == msg, (v["source"], kind, msg)
        assert got == out and (bits + 7) // 8 == used, (v["source"], bits, used)


def test_inflate_ref_on_system_zlib_streams(o):
    for cls in range(8):
        raw = o.gen_shard(cls, 20000)
        for level in (1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            s = c.compress(raw) + c.flush()
            st, out, bits, kind = D.inflate_ref(s, len(raw))
            assert (st, out, (bits + 7) // 8, kind) == (0, raw, len(s), None), (cls, level)
            st, out, bits, kind = D.inflate_ref(s[:len(s) // 2], len(raw))
            rc, want, used, _ = o.inflate(s[:len(s) // 2], len(raw), 0)
            assert (st, out, (bits + 7) // 8, kind) == (rc, want, used, "need input"), (cls, level)
            st, out, bits, kind = D.inflate_ref(s, len(raw) - 1)
            rc, want, used, _ = o.inflate(s, len(raw) - 1, 0)
            assert (st, out, (bits + 7) // 8, kind) == (rc, want, used, "need room"), (cls, level)


def test_valid_streams_agree_with_expand_zlib_and_the_oracle(o):
    """expand, inflate_ref, system zlib and the oracle give the same bytes; status, bytes and bytes used of inflate_ref are the
    oracle's; the streams have the sizes they are meant to have"""
    cases = K.valid() + K.exact_distance()
    for c in cases:
        assert zlib.decompress(c.stream, -15) == c.raw, c.name
        rc, out, used, msg = o.inflate(c.stream, len(c.raw), 0)
        assert (rc, out, used) == (1, c.raw, len(c.stream)), (c.name, rc, msg)
        assert K.expected(c, len(c.raw)) == (0, c.raw, len(c.stream), None), c.name
    by = {c.name: c for c in cases}
    fast = [c for c in cases if len(c.stream) > 4200]
    assert len(fast) >= 18 and all(len(c.stream) < 64 << 10 for c in cases), [(c.name, len(c.stream)) for c in cases if len(c.stream) >= 64 << 10]
    assert len(by["headers"].blocks) == 40 and len(by["tiny_blocks"].blocks) == 300
    assert sum(1 for at in by["headers"].blocks if at & 7) > 20
    assert len(by["worst_tables/40"].stream) < 1024


def test_the_headers_have_the_shapes_they_are_meant_to_have():
    ll, dl = K.worst_codes(851)
    size = {}
    for shape in ("plain", "rle", "long", "min"):
        b = D._Bits()
        D.dynamic_block([], ll, dl, bits=b, header=shape)
        size[shape] = D._pos(b)
        assert zlib.decompress(b.finish(), -15) == b""
    assert size["long"] > size["plain"] > size["rle"] and size["long"] > 17 + 19 * 3 + 316 * 6
    for codes, shape, hclen in (((K.HCLEN5, [0]), "min", 5), (K.wide_codes(), "plain", 19)):
        b = D._Bits()
        D.dynamic_block([], codes[0], codes[1], bits=b, header=shape)
        assert (int.from_bytes(b.finish()[:3], "little") >> 13 & 15) + 4 == hclen
    # a repeat that starts in the literal/length lengths and ends in the distance lengths
    ll, dl = [8] * 255 + [0, 8] + [0] * 20, [0] * 10 + [1, 1]
    assert D._cl_symbols(ll + dl, "rle")[-3:] == [(18, 30 - 11, 7), (1, 0, 0), (1, 0, 0)]
    b = D._Bits()
    D.dynamic_block([65], ll, dl, bits=b)
    assert zlib.decompress(b.finish(), -15) == b"A"


def test_failing_streams_fail_as_intended(o):
    """for every error class the oracle reports the intended message on at least one stream; no stream of the failing list decodes
    cleanly; status, bytes and bytes used of inflate_ref are the oracle's on every one of them; the unused half of a
    single-code form is a data error with one bit in hand and one bit read (inftrees.rs:61-67, :230-241), cut or not"""
    cases = K.failing()
    seen = {}
    for c in cases:
        rc, out, used, msg = o.inflate(c.stream, K.AMPLE, 0)
        st, got, nbytes, kind = K.expected(c)
        assert rc not in (0, 1) and st != 0, (c.name, rc)
        assert (st, got, nbytes, K.MESSAGE[kind]) == (rc, out, used, msg), (c.name, st, rc, nbytes, used, kind, msg)
        with pytest.raises(zlib.error):
            zlib.decompress(c.stream, -15)
        seen.setdefault(c.klass, set()).add(kind)
        if "/cut " not in c.name and c.klass in K.CLASSES:
            assert kind == K.CLASSES[c.klass][1], (c.name, kind)
            assert c.bad is None or (c.bad > 8 * 8192 if "/deep" in c.name else c.bad < 8 * 200), (c.name, c.bad)
        if c.klass.startswith("unused code"):
            assert (st, kind, nbytes) == (K.Z_DATA_ERROR, K.CLASSES[c.klass][1], c.bad // 8 + 1), (c.name, st, kind, nbytes)
    for klass, (_, kind) in K.CLASSES.items():
        assert kind in seen[klass], klass
    assert {k for _, k in K.CLASSES.values()} >= set(D.KINDS) - {"invalid block type", "stored lengths", "need input", "need room"}
    last = [c for c in cases if c.klass == "cut behind a 48-bit token"][0]
    assert K.expected(last)[:3] == (K.Z_BUF_ERROR, last.prefix, len(last.stream)) and last.prefix[-258:] == last.prefix[-258 - 32768:-32768]
    for good, bad in K.history_pairs():
        assert D.inflate_ref(good.stream, K.AMPLE, 0, good.hist)[:2] == (0, good.raw)
        assert D.inflate_ref(good.stream, K.AMPLE, 0, good.hist[1:])[::3] == (K.Z_DATA_ERROR, "distance too far back")
        assert bad is None or D.inflate_ref(bad.stream, K.AMPLE, 0, bad.hist)[::3] == (K.Z_DATA_ERROR, "distance too far back")
