"""Checks of batch deflate and inflate against one shared preset dictionary: zmi_deflate_batch_shared_dict_dev,
zmi_inflate_batch_shared_dict_dev and zmi_deflate_dict_bound (include/zmi355.h; csrc/lz77.hip, encode.hip, inflate.hip,
zmi_api.hip).  Shared by the emulator tests (CPU, tests/test_emu_shared_dict.py) and the -m gpu tests
(tests/test_gpu_shared_dict.py).  The judge is Python's zlib module (the system zlib): what this library compresses,
zlib.decompressobj(zdict=...) must read back; what zlib.compressobj(zdict=...) writes, this library must decode.

A target is an object with these methods, all on host data (the adapter moves it to where the library reads it):
  deflate(shards, level, strategy, wrap, zdict, dict_align=0, in_align=0, stride=None, max_len=None, plain=False, null_dict=False)
      -> (rc, [stream bytes], [status], guards_untouched)
      shards: list of bytes, packed back to back from an address = in_align (mod 16); zdict: bytes at an address = dict_align
      (mod 16); plain: zmi_deflate_batch_dev instead (zdict ignored); null_dict: d_dict = NULL with dict_len = len(zdict).  The
      output buffer is filled with 0xA5 before the call; guards_untouched: every byte from a stream's length rounded up to 16 to
      the end of its slot, and 64 bytes behind the last slot, still hold it.  stride None = the call's bound of max_len.
  inflate(streams, wrap, zdict, caps, dict_align=0, gap=1) -> (rc, [output bytes], [out_len], [status], [in_used], guards_untouched)
      output regions packed back to back from an odd address with `gap` guard bytes (0xEE) between them
  dict_bound(n, wrap), bound(n, wrap), set_scratch_limit(bytes)
"""
import lzma
import os
import struct
import zlib

import numpy as np

import deflate_craft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW, ZLIB, GZIP, AUTO = 0, 1, 2, 3
WBITS = {RAW: -15, ZLIB: 15}
E_ARG = -103

DICT_LENS = [1, 15, 16, 17, 262, 1023, 1024, 1025, 4101, 27632, 27648, 27649, 32768, 40000]
DICT_ALIGNS = [0, 1, 7]
SMALL_LENS = [0, 1, 3, 4, 5, 6, 258, 1000, 1024, 4096]
BIG_LEN = 70000           # crosses a 64 KiB encoder piece and lets the dictionary leave the window
INF_DICT_LENS = [1, 17, 1024, 1025, 32768, 40000]
# (level, strategy): levels 1, 6, 9 at both wraps, and one launch each for level 0, Z_HUFFMAN_ONLY and Z_RLE
DEFLATE_CONFIGS = [(1, 0, RAW), (1, 0, ZLIB), (6, 0, RAW), (6, 0, ZLIB), (9, 0, RAW), (9, 0, ZLIB), (0, 0, ZLIB), (6, 2, ZLIB), (6, 3, RAW)]

_TEXT = None


def text():
    global _TEXT
    if _TEXT is None:
        with lzma.open(os.path.join(ROOT, "tests", "golden", "fixtures", "lcet10.txt.xz")) as f:
            _TEXT = f.read()
    return _TEXT


def text_case(dict_len, lens):
    """dictionary = a prefix of the text, shards = slices behind it"""
    t = text()
    shards, at = [], max(dict_len, 40000)
    for n in lens:
        shards.append(t[at:at + n])
        at += n + 13
    return t[:dict_len], shards


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def read_back(stream, wrap, zdict, want, what):
    """zlib.decompressobj(-15 | 15, zdict) returns the shard, reaches the end of the stream and leaves nothing over; for the zlib
    wrapper this also proves FDICT, FCHECK and the DICTID (zlib asks for the dictionary by it)"""
    d = zlib.decompressobj(WBITS[wrap], zdict=zdict) if zdict else zlib.decompressobj(WBITS[wrap])
    got = d.decompress(stream)
    assert got == want and d.eof and d.unused_data == b"", what


def check_header(stream, zdict):
    assert stream[0] == 0x78 and (stream[1] & 0x20) and ((stream[0] << 8) | stream[1]) % 31 == 0
    assert struct.unpack(">I", stream[2:6])[0] == zlib.adler32(zdict)


# ---- what both adapters do with the buffers after a call -------------------------------------------------------------------
def collect_deflate(rc, out, stride, olen, st, n, max_len):
    """out: u8 array of n * stride + 64 bytes that held 0xA5 before the call.  Guards: the 64 bytes behind the last slot; in a
    launch whose shards are one encoder piece each (max_len <= 64 KiB: a slot is written front to back) also every byte from a
    stream's length rounded up to 16 to the end of its slot.  (With several pieces the encoder parks the later ones further
    back in the slot before it closes the gaps.)"""
    if rc != 0:
        return rc, [], [], False
    outs, guards = [], bool((out[n * stride:] == 0xA5).all())
    for i in range(n):
        ln = int(olen[i])
        outs.append(bytes(out[i * stride:i * stride + ln]))
        guards = guards and ln <= stride
        if max_len <= 65536:
            guards = guards and bool((out[i * stride + ((ln + 15) & ~15):(i + 1) * stride] == 0xA5).all())
    return rc, outs, [int(x) for x in st], guards


def region_layout(caps, gap):
    """output regions back to back with `gap` guard bytes between them -> (u64 offsets, bytes needed)"""
    ooff, at = np.zeros(len(caps), dtype=np.uint64), gap
    for i, c in enumerate(caps):
        ooff[i] = at
        at += c + gap
    return ooff, at + 64


def collect_inflate(rc, out, ooff, caps, olen, st, used, gap):
    """out: u8 array that held 0xEE before the call"""
    if rc != 0:
        return rc, [], [], [], [], False
    outs, mask = [], np.ones(out.size, dtype=bool)
    for i, c in enumerate(caps):
        o = int(ooff[i])
        outs.append(bytes(out[o:o + min(int(olen[i]), c)]))
        mask[o:o + c] = False
    return rc, outs, [int(x) for x in olen], [int(x) for x in st], [int(x) for x in used], bool((out[mask] == 0xEE).all())


# ---- deflate -------------------------------------------------------------------------------------------------------------
def _round_trip(target, shards, level, strategy, wrap, zdict, dict_align, in_align, what):
    max_len = max([len(s) for s in shards] + [1])
    rc, outs, sts, guards = target.deflate(shards, level, strategy, wrap, zdict, dict_align=dict_align, in_align=in_align)
    assert rc == 0, what
    for i, (s, o, st) in enumerate(zip(shards, outs, sts)):
        w = (what, i, len(s))
        assert st == 0, w
        assert len(o) <= target.dict_bound(len(s), wrap) <= target.dict_bound(max_len, wrap), w
        if wrap == ZLIB:
            check_header(o, zdict)
        read_back(o, wrap, zdict, s, w)
    assert guards, what
    return outs


def deflate_matrix(target, level, strategy, wrap, dict_lens=DICT_LENS, aligns=DICT_ALIGNS, big=True):
    """check 1: round trip over dictionary length x dictionary alignment x shard length; returns the number of shards checked
    and, for check 10, [(dictionary, wrap, shards, streams)]"""
    n, kept = 0, []
    for dl in dict_lens:
        for k, a in enumerate(aligns):
            zdict, shards = text_case(dl, SMALL_LENS)
            what = (level, strategy, wrap, dl, a)
            outs = _round_trip(target, shards, level, strategy, wrap, zdict, a, (3 + 5 * k) % 16, what)
            n += len(shards)
            kept.append((zdict, wrap, shards, outs))
            if big and a == aligns[0]:
                zdict, shards = text_case(dl, [BIG_LEN, 1000])
                outs = _round_trip(target, shards, level, strategy, wrap, zdict, a, 9, what + ("big",))
                n += len(shards)
                kept.append((zdict, wrap, shards, outs))
    return n, kept


def deflate_seam(target, level=6):
    """check 2: matches that start in the dictionary and run into the shard"""
    t = text()
    p50 = t[50000:50050]
    body = t[:3000]
    tail300 = random_bytes(300, 5)
    cases = [
        (body + p50, p50 * 10),
        (body + b"xyz" * 40, b"xyz" * 200),
        (body + tail300, tail300 + random_bytes(300, 6)),
    ]
    n = 0
    for wrap in (RAW, ZLIB):
        for a, (zdict, shard) in zip(DICT_ALIGNS, cases):
            outs = _round_trip(target, [shard, shard[:7], shard], level, 0, wrap, zdict, a, 5, ("seam", wrap, a))
            assert outs[0] == outs[2]
            # the third shard's second half is random: only its first 300 bytes, the dictionary's tail, can shrink -- to a few
            # tokens if the match across the seam is found, to nothing otherwise
            assert len(outs[0]) < len(shard) - 200, (len(outs[0]), len(shard))
            n += 1
    return n


def deflate_uses_dictionary(target, level=6):
    """check 3: 4096-byte slices of a random dictionary's last 16 KiB.  Without the dictionary random bytes do not shrink; with it a
    shard is sixteen 258-byte matches and a block header -- well under 200 bytes -- so out_len < len / 4 is a condition, not a
    measurement"""
    zdict = random_bytes(32768, 11)
    shards = [zdict[32768 - 16384 + k:32768 - 16384 + k + 4096] for k in (0, 1, 4097, 8191, 12288)]
    for wrap in (RAW, ZLIB):
        rc, plain, sts, _ = target.deflate(shards, level, 0, wrap, None, plain=True)
        assert rc == 0 and all(st == 0 for st in sts)
        assert all(len(o) >= len(s) for o, s in zip(plain, shards))
        outs = _round_trip(target, shards, level, 0, wrap, zdict, 7, 3, ("uses", wrap))
        for o, s in zip(outs, shards):
            assert len(o) < len(s) // 4, (len(o), len(s))
    return len(shards)


# check 4: what the emulator measured (tests/test_emu_shared_dict.py::test_ratio_on_text prints it; profiles/shared_dict.json holds
# it): total compressed size of 64 text records of 4 KiB behind a 32 KiB text dictionary, against zlib.compressobj(level,
# DEFLATED, -15, zdict=dict) on the same records, in per cent.  The gate is that plus 1.5 points, the slack of the project's other
# ratio gates (tests/test_gpu_parity.py).  The bytes are the same on the emulator and on the GPU.
RATIO_EXCESS_MEASURED = {6: 1.15, 9: 0.25}
RATIO_SLACK = 1.5


def ratio_records(n=64, size=4096):
    t = text()
    zdict = t[:32768]
    return zdict, [t[32768 + i * size:32768 + (i + 1) * size] for i in range(n)]


def deflate_ratio(target, level):
    """-> (excess over zlib in per cent, total with the dictionary, total without, zlib's total)"""
    zdict, recs = ratio_records()
    rc, outs, sts, _ = target.deflate(recs, level, 0, RAW, zdict)
    assert rc == 0 and all(st == 0 for st in sts)
    for o, r in zip(outs, recs):
        read_back(o, RAW, zdict, r, level)
    rc, plain, sts, _ = target.deflate(recs, level, 0, RAW, None, plain=True)
    assert rc == 0 and all(st == 0 for st in sts)
    ref = 0
    for r in recs:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=zdict)
        ref += len(co.compress(r) + co.flush())
    ours, without = sum(len(o) for o in outs), sum(len(o) for o in plain)
    return 100.0 * (ours - ref) / ref, ours, without, ref


def deflate_equalities(target):
    """check 5: no dictionary = zmi_deflate_batch_dev byte for byte; a shard's bytes depend on the dictionary and the shard alone"""
    zdict, shards = text_case(4101, [1000, 0, 4096, 5, 70000])
    n = 0
    for wrap in (RAW, ZLIB):
        rc0, base, st0, _ = target.deflate(shards, 6, 0, wrap, None, plain=True)
        rc1, a, st1, g1 = target.deflate(shards, 6, 0, wrap, b"", stride=target.bound(70000, wrap))
        rc2, b, st2, g2 = target.deflate(shards, 6, 0, wrap, zdict, null_dict=True, stride=target.bound(70000, wrap))
        assert rc0 == rc1 == rc2 == 0 and st0 == st1 == st2 and base == a == b and g1 and g2, wrap
        n += 2
    zdict, _ = text_case(32768, [])
    shard = text()[60000:64096]
    for wrap in (RAW, ZLIB):
        rc, one, st, _ = target.deflate([shard], 6, 0, wrap, zdict, dict_align=0, in_align=0)
        assert rc == 0 and st == [0]
        others = [text()[70000 + 4096 * i:70000 + 4096 * (i + 1)] for i in range(64)]
        others[37] = shard
        rc, many, st, _ = target.deflate(others, 6, 0, wrap, zdict, dict_align=7, in_align=11)
        assert rc == 0 and many[37] == one[0], wrap
        # a scratch limit that forces several launch groups: 64 MiB is the smallest the context takes; 4 KiB shards inside a
        # max_len of 1 MiB take 4.25 MiB of scratch each, 15 to a group
        target.set_scratch_limit(64 << 20)
        try:
            rc, grouped, st, _ = target.deflate(others, 6, 0, wrap, zdict, dict_align=1, in_align=5, max_len=1 << 20)
            rc2, single, st2, _ = target.deflate([shard], 6, 0, wrap, zdict, max_len=1 << 20)
        finally:
            target.set_scratch_limit(8 << 30)
        assert rc == 0 and rc2 == 0 and all(x == 0 for x in st) and grouped[37] == single[0], wrap
        read_back(grouped[37], wrap, zdict, shard, wrap)
        n += 3
    return n


def deflate_arguments(target):
    """check 6"""
    zdict, shards = text_case(1024, [1000])
    for wrap in (GZIP, AUTO):
        rc, _, _, _ = target.deflate(shards, 6, 0, wrap, zdict, stride=target.dict_bound(1000, ZLIB) + 32)
        assert rc == E_ARG, wrap
    for n in (0, 1, 8, 9, 1000, 4096, 70000, 1 << 20):
        raw = n + (n == 0) + (n < 9) + ((n + 7) >> 3) + 3
        assert target.dict_bound(n, ZLIB) == (raw + 6 + 4 + 15) // 16 * 16 and target.dict_bound(n, RAW) == (raw + 15) // 16 * 16 == target.bound(n, RAW)
    # a length whose plain bound, rounded up to 16, leaves no room for the DICTID
    n = next(k for k in range(1, 64) if target.dict_bound(k, ZLIB) > target.bound(k, ZLIB))
    zdict, shards = text_case(1024, [n])
    rc, _, _, _ = target.deflate(shards, 6, 0, ZLIB, zdict, stride=target.bound(n, ZLIB))
    assert rc == E_ARG
    rc, outs, sts, _ = target.deflate(shards, 6, 0, ZLIB, zdict, stride=target.dict_bound(n, ZLIB))
    assert rc == 0 and sts == [0]
    read_back(outs[0], ZLIB, zdict, shards[0], n)
    return 4


# ---- inflate -------------------------------------------------------------------------------------------------------------
def zlib_stream(data, level, wrap, zdict):
    co = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap], zdict=zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap])
    return co.compress(data) + co.flush()


def _decode(target, streams, wants, wrap, zdict, dict_align, what, slack=0):
    caps = [len(w) + slack for w in wants]
    rc, outs, olens, sts, used, guards = target.inflate(streams, wrap, zdict, caps, dict_align=dict_align)
    assert rc == 0, what
    for i, (s, w) in enumerate(zip(streams, wants)):
        assert sts[i] == 0 and olens[i] == len(w) and outs[i] == w and used[i] == len(s), (what, i, sts[i], olens[i], len(w), used[i], len(s))
    assert guards, what
    return len(streams)


def inflate_matrix(target, level, wrap, dict_lens=INF_DICT_LENS, aligns=DICT_ALIGNS, big=True):
    """check 7: zlib's own streams (it reaches about 32 506 bytes back, further than this library's encoder) over dictionary
    length x alignment x shard length, regions packed back to back: a decoder that still reads in front of a region reads
    its neighbour and fails"""
    n = 0
    for dl in dict_lens:
        for a in aligns:
            zdict, shards = text_case(dl, SMALL_LENS + ([BIG_LEN] if big and a == aligns[0] else []))
            if dl == 32768:
                shards.append(zdict[:300])    # the distance of its first match is about 32 768
            shards = shards + shards          # (more than 16 streams: both decode kernels of the `inf_selection` fixture get the launch)
            streams = [zlib_stream(s, level, wrap, zdict) for s in shards]
            n += _decode(target, streams, shards, wrap, zdict, a, (level, wrap, dl, a))
    return n


def inflate_crafted(target):
    """check 8: first tokens that reach into the dictionary, to its first byte, and one byte in front of it"""
    n = 0
    for dl in (3, 300, 1024, 32767):
        zdict = random_bytes(dl, 20 + dl)
        for a in (0, 7):
            cases = [[(258, 3), 65, (5, 2)], [(min(258, dl), dl)], [66, (3, dl + 1), 67]]
            if dl >= 300:   # a source further back than the resolve pass keeps in LDS that starts in the dictionary and ends in the output
                cases.append(list(random_bytes(1700, 9)) + [(258, 1800), 7, (100, 1900)])
            if dl > 2000:   # ... and one that lies in the dictionary
                cases.append([1, 2, 3, (200, dl - 100), (258, 1800)])
            too_far = deflate_craft.fixed_block([(3, dl + 1)])
            streams = [deflate_craft.fixed_block(t) for t in cases]
            wants = [zlib.decompressobj(-15, zdict=zdict).decompress(s) for s in streams]
            rc, outs, olens, sts, used, guards = target.inflate(streams + [too_far], RAW, zdict, [len(w) + 3 for w in wants] + [64], dict_align=a)
            assert rc == 0 and guards
            for i, w in enumerate(wants):
                assert sts[i] == 0 and outs[i] == w and used[i] == len(streams[i]), (dl, a, i, sts[i])
            assert wants[0][:6] == (zdict[-3:] * 2)[:6] and wants[1] == zdict[:len(wants[1])]
            assert sts[len(wants)] == -3, (dl, a, sts)
            try:   # ... and zlib says the same of that stream
                zlib.decompressobj(-15, zdict=zdict).decompress(too_far)
                raise AssertionError("zlib accepted a distance in front of the dictionary")
            except zlib.error:
                pass
            n += 1
    return n


def inflate_status_mix(target):
    """check 9: right DICTID, wrong DICTID (-3), FDICT in a call without dictionary (2), no FDICT (0), truncated (-5), and the
    neighbours of every failing stream still correct"""
    zdict, shards = text_case(4101, [1000, 1024, 4096, 1000, 258, 1000, 4096])
    other = text()[90000:94101]
    good = [zlib_stream(s, 6, ZLIB, zdict) for s in shards]
    wrong = zlib_stream(shards[1], 6, ZLIB, other)
    nofdict = zlib_stream(shards[3], 6, ZLIB, None)
    streams = [good[0], wrong, good[2], nofdict, good[4], good[5][:len(good[5]) // 2], good[6]]
    caps = [len(s) for s in shards]
    rc, outs, olens, sts, used, guards = target.inflate(streams, ZLIB, zdict, caps, dict_align=1)
    assert rc == 0 and guards
    assert sts == [0, -3, 0, 0, 0, -5, 0], sts
    for i in (0, 2, 3, 4, 6):
        assert outs[i] == shards[i] and olens[i] == len(shards[i]) and used[i] == len(streams[i]), i
    assert olens[1] == 0
    rc, outs, olens, sts, used, guards = target.inflate([nofdict, good[0], nofdict], ZLIB, b"", [len(shards[3]), len(shards[0]), len(shards[3])])
    assert rc == 0 and guards and sts == [0, 2, 0], sts
    assert outs[0] == shards[3] and outs[2] == shards[3]
    for wrap in (GZIP, AUTO):
        rc = target.inflate([good[0]], wrap, zdict, [caps[0]])[0]
        assert rc == E_ARG, wrap
    return 7


def inflate_own_output(target, kept):
    """check 10: the streams of check 1 through the new inflate"""
    n = 0
    for zdict, wrap, shards, streams in kept:
        n += _decode(target, streams, shards, wrap, zdict, 7, ("own", wrap, len(zdict)))
    return n
