"""Checks of the multi-member gzip calls (zmi_gzip_find_members_dev / zmi_inflate_members_dev, include/zmi355.h), shared by
tests/test_emu_members.py (CPU, the emulator build through ctypes) and tests/test_gpu_members.py (the MI355X through Engine).

The judge is Python's zlib / gzip on the CPU, which reads multi-member files; the library's own inflate never judges alone.

A target offers
    find(data, cap=None, shift=0)       -> list of proposed starts (the data placed `shift` bytes behind a 16-byte boundary)
    raw(data, starts, out_cap)          -> Result of ONE zmi_inflate_members_dev call (starts None: find's list)
    all(data, starts=None)              -> (bytes, member offsets) of the whole file, continuing behind ZMI_MM_AGAIN
    own_members(shards)                 -> the gzip members this library's deflate_batch (level 6) makes of the shards
    pack(members)                       -> (the stitched file, offsets) through zmi_pack_slab_dev
    set_group_limit(nbytes or None)     -> the limit that cuts launch groups: the tuning override ZMI_MM_LIMIT (the scratch limit's floor is
                                           64 MiB, above these files); None: the context's scratch limit again
"""
import gzip
import itertools
import random
import struct
import zlib

HEADER, TRUNC, DATA, CHECK, LENGTH, OUT, BIG, AGAIN = 1, 2, 3, 4, 5, 6, 7, 8
Z_DATA_ERROR, Z_BUF_ERROR, E_ARG = -3, -5, -103
GUARD = 64          # bytes behind out_cap every raw() call watches
FILL = 0xC7

LENS = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 70000]
LEVELS = [0, 1, 6, 9]
COUNTS = [1, 2, 3, 300]


class Result:
    def __init__(self, rc, status, detail, members, in_used, out_len, out, guard_ok, member_off):
        self.rc, self.status, self.kind, self.index = rc, status, detail & 0xFF, (detail & 0xFFFFFFFF) >> 8
        self.members, self.in_used, self.out_len, self.out, self.guard_ok, self.member_off = members, in_used, out_len, out, guard_ok, member_off

    def __repr__(self):
        return "Result(rc=%d status=%d kind=%d index=%d members=%d in_used=%d out_len=%d)" % (self.rc, self.status, self.kind, self.index,
                                                                                              self.members, self.in_used, self.out_len)


# ---- building files ---------------------------------------------------------------------------------------------------------
def text(n, seed):
    """n compressible bytes (words of a small vocabulary, some noise)"""
    r = random.Random(seed)
    words = [bytes(r.randrange(97, 123) for _ in range(r.randrange(2, 9))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + (b" " if r.random() < 0.9 else bytes([r.randrange(256)]))
    return bytes(out[:n])


def member(raw, level=6, fextra=None, fname=None, fcomment=None, fhcrc=False, mtime=0):
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + b"\x00\x03"
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return h + c.compress(raw) + c.flush() + struct.pack("<II", zlib.crc32(raw), len(raw) & 0xFFFFFFFF)


def starts_of(members):
    s, at = [], 0
    for m in members:
        s.append(at)
        at += len(m)
    return s


def byte_search(data):
    """the filter of zmi_gzip_find_members_dev, byte by byte"""
    out = [0] if data else []
    p = data.find(b"\x1f\x8b\x08", 1)
    while p >= 0 and p + 18 <= len(data):
        if data[p + 3] & 0xE0 == 0:
            out.append(p)
        p = data.find(b"\x1f\x8b\x08", p + 1)
    return out


def judge(data):
    """(output, member output offsets, input bytes the members cover) by zlib: members are read while one starts where the last ended"""
    out, offs, at = bytearray(), [], 0
    while at < len(data):
        d = zlib.decompressobj(31)
        try:
            piece = d.decompress(data[at:])
        except zlib.error:
            break
        if not d.eof:
            break
        offs.append(len(out))
        out += piece
        at = len(data) - len(d.unused_data)
    return bytes(out), offs + [len(out)], at


def zlib_case(data):
    """how zlib fails on the member at the start of `data`: the ZMI_MM_* case"""
    d = zlib.decompressobj(31)
    try:
        d.decompress(data)
    except zlib.error as e:
        msg = str(e)
        if "incorrect header check" in msg or "unknown compression method" in msg or "unknown header flags" in msg:
            return HEADER
        if "incorrect data check" in msg:
            return CHECK
        if "incorrect length check" in msg:
            return LENGTH
        return DATA
    return 0 if d.eof else TRUNC


def expect_file(target, data, starts=None, want=None):
    """the whole file through the target equals the judge's reading"""
    ref, offs, covered = judge(data)
    if want is not None:
        assert ref == want
    got, moff = target.all(data, starts)
    assert got == ref, (len(got), len(ref))
    assert list(moff) == offs
    return len(offs) - 1


def one_call(target, data, starts=None, slack=4096):
    """one raw call with room for the judge's output + slack; the guard bytes must survive"""
    ref, offs, covered = judge(data)
    r = target.raw(data, starts, len(ref) + slack)
    assert r.rc == 0 and r.guard_ok, r
    return r, ref, offs, covered


def expect_complete(r, ref, offs, covered):
    assert r.status == 0 and r.kind == 0, r
    assert r.members == len(offs) - 1 and r.out_len == len(ref) and r.in_used == covered, r
    assert r.out[:r.out_len] == ref
    assert r.member_off[:r.members + 1] == offs


def expect_prefix(r, data, ref, offs):
    """whatever the status: the verified prefix is right and ends on a true member boundary"""
    assert r.members <= len(offs) - 1, r
    assert r.out_len == offs[r.members] or r.kind == OUT, r
    assert r.out[:offs[r.members]] == ref[:offs[r.members]]
    assert r.member_off[:r.members + 1] == offs[:r.members + 1]
    _, _, covered = judge(data[:r.in_used])
    assert covered == r.in_used, r


# ---- 1. exactness of the scan ---------------------------------------------------------------------------------------------------
def scan_files(target, counts=COUNTS, own=True):
    """files of `counts` members, raw lengths LENS in turn, levels 0 / 1 / 6 / 9 in turn (and this library's own members)"""
    files = []
    for n in counts:
        raws = [text(LENS[(i + n) % len(LENS)], 100 * n + i) for i in range(n)]
        files.append(b"".join(member(r, LEVELS[i % 4]) for i, r in enumerate(raws)))
    if own:
        raws = [text(l, 7000 + l) for l in LENS]
        files.append(b"".join(target.own_members(raws)))
    return files


def scan_exactness(target, counts=COUNTS, own=True):
    done = 0
    for data in scan_files(target, counts, own):
        want = byte_search(data)
        got = target.find(data)
        assert got == want, (len(got), len(want))
        assert target.find(data) == got                      # the same list on every run
        assert target.find(data, shift=5) == want            # ... at any address
        if len(want) > 1:
            cap = len(want) // 2
            assert target.find(data, cap=cap) == want[:cap]  # a cap keeps the first entries
        done += 1
    assert target.find(b"") == []
    m = member(b"", 6)
    assert len(m) == 20
    assert target.find(m[:17]) == [0]
    assert target.find(m[:2] + m[:18]) == [0, 2]             # exactly 18 bytes from the last start to the end
    assert target.find(m[:2] + m[:17]) == [0]                # 17
    # more than 200 members inside one 4 KiB stretch
    many = m * 230
    assert target.find(many) == [20 * i for i in range(230)]
    return done


# ---- 2. boundary straddles ------------------------------------------------------------------------------------------------------
STRADDLE_AROUND = [96, 1024, 4096, 16384]   # a 16-byte line, a wave of lines, 4 KiB, the scan's 16 KiB segment


def straddles(target, arounds=STRADDLE_AROUND, deltas=range(-6, 5), decode=True):
    done = 0
    b = member(text(300, 1), 6)
    c = member(text(17, 2), 1)
    for around in arounds:
        for d in deltas:
            at = around + d
            a = member(text(40, at), 6, fname=b"n" * (at - len(member(text(40, at), 6)) - 1))
            assert len(a) == at
            data = a + b + c
            want = byte_search(data)
            assert at in want and at + len(b) in want
            got = target.find(data)
            assert got == want, (at, got, want)
            assert target.find(data, shift=9) == want
            if decode:
                assert expect_file(target, data) == 3
            done += 1
    return done


# ---- 3. header fields -----------------------------------------------------------------------------------------------------------
def header_fields(target):
    bgzf = b"BC" + struct.pack("<HH", 2, 0x1234)
    ms = []
    for i, (fx, fn, fc, fh, mt) in enumerate(itertools.product([None, bgzf + b"XY\x03\x00abc"], [None, b"file-name.txt"], [None, b"a comment"],
                                                                [False, True], [0, 0x5F3759DF])):
        ms.append(member(text(100 + 37 * i, i), LEVELS[i % 4], fextra=fx, fname=fn, fcomment=fc, fhcrc=fh, mtime=mt))
        ms.append(member(text(50 + i, 500 + i), 6))
    data = b"".join(ms)
    assert gzip.decompress(data) == judge(data)[0]
    r, ref, offs, covered = one_call(target, data)
    expect_complete(r, ref, offs, covered)
    assert expect_file(target, data) == 64
    return len(ms)


# ---- 4. round trip of the project's own output ------------------------------------------------------------------------------------
def own_round_trip(target, n=64, shard=65536, low_limit=None):
    shards = [text(shard, 9000 + i) for i in range(n)]
    members = target.own_members(shards)
    data, off = target.pack(members)
    assert data == b"".join(members) and off[-1] == len(data)
    ref, offs, covered = judge(data)
    assert ref == b"".join(shards) and offs == [shard * i for i in range(n + 1)] and covered == len(data)
    r = target.raw(data, None, len(ref))
    expect_complete(r, ref, offs, covered)
    assert r.members == n and r.guard_ok
    if low_limit is not None:
        # out_cap above the limit: out_cap / (limit / 2) + 1 launch groups per pass (include/zmi355.h)
        assert len(ref) // (low_limit // 2) + 1 >= 3
        target.set_group_limit(low_limit)
        try:
            r2 = target.raw(data, None, len(ref))
        finally:
            target.set_group_limit(None)
        expect_complete(r2, ref, offs, covered)
        assert r2.out == r.out and r2.member_off == r.member_off
        assert (r2.status, r2.kind, r2.index, r2.members, r2.in_used, r2.out_len) == (r.status, r.kind, r.index, r.members, r.in_used, r.out_len)
    return n


# ---- 5. false proposals -----------------------------------------------------------------------------------------------------------
BAIT = b"\x1f\x8b\x08\x00" + b"\x00" * 20   # a header image: passes the filter, decodes to nothing good


def _stored(payload_parts, seed):
    raw = b"".join(payload_parts)
    m = member(raw, 0)
    assert raw in m                          # level 0: the payload stands in the member as it is
    return m, raw


def false_proposals(target, cases="abcde"):
    done = 0
    plain = [member(text(900 + 13 * i, 40 + i), LEVELS[i % 4]) for i in range(6)]
    if "a" in cases:    # one header image in one member: one call
        m, _ = _stored([text(500, 1), BAIT, text(700, 2)], 1)
        data = b"".join(plain[:2] + [m] + plain[2:])
        assert len(byte_search(data)) == 8
        r, ref, offs, covered = one_call(target, data)
        expect_complete(r, ref, offs, covered)
        expect_complete(target.raw(data, None, len(ref)), ref, offs, covered)    # ... with no room to spare
        done += 1
    if "b" in cases:    # a complete small gzip file inside a stored member: the false proposal decodes cleanly on its own
        inner = member(text(200, 3), 6)
        assert judge(inner)[0] == text(200, 3)
        m, _ = _stored([text(300, 5), inner, text(400, 6)], 2)
        data = b"".join(plain[:3] + [m] + plain[3:])
        assert len(byte_search(data)) == 8
        r, ref, offs, covered = one_call(target, data)
        expect_complete(r, ref, offs, covered)
        done += 1
    if "c" in cases:    # two baits in one member, baits in two adjacent members: AGAIN is allowed, the loop completes
        m2, _ = _stored([text(300, 7), BAIT, text(300, 8), BAIT, text(300, 9)], 3)
        ma, _ = _stored([text(200, 10), BAIT, text(200, 11)], 4)
        mb, _ = _stored([text(250, 12), BAIT, text(150, 13)], 5)
        for data in (b"".join([m2] + plain), b"".join(plain[:2] + [m2] + plain[2:]), b"".join(plain[:1] + [ma, mb] + plain[1:])):
            r, ref, offs, covered = one_call(target, data)
            if r.status != 0:
                assert (r.status, r.kind) == (Z_BUF_ERROR, AGAIN) and r.members >= 1, r
                expect_prefix(r, data, ref, offs)
            else:
                expect_complete(r, ref, offs, covered)
            expect_file(target, data)
            done += 1
    if "d" in cases:    # a caller's list with a bogus start in the middle of Huffman data
        big = member(text(5000, 14), 6)
        data = b"".join(plain[:2] + [big] + plain[2:])
        st = starts_of(plain[:2] + [big] + plain[2:])
        bogus = sorted(st + [st[2] + len(big) // 2])
        r, ref, offs, covered = one_call(target, data, bogus)
        expect_complete(r, ref, offs, covered)
        done += 1
    if "e" in cases:    # a caller's list that misses a true start (in the middle; the last one)
        data = b"".join(plain)
        st = starts_of(plain)
        for drop in (3, 5):
            lst = st[:drop] + st[drop + 1:]
            r, ref, offs, covered = one_call(target, data, lst)
            assert r.status == 0 or (r.status, r.kind) == (Z_BUF_ERROR, AGAIN), r
            assert r.members >= 1
            expect_prefix(r, data, ref, offs)
            assert (r.status == 0) == (drop == 5)             # nothing left in the list to try / something left
            # continuing from *d_in_used finishes the file
            rest = data[r.in_used:]
            assert rest and rest == data[st[r.members]:]
            got, _ = target.all(rest, None)
            assert r.out[:r.out_len] + got == ref
            done += 1
    return done


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def _twelve():
    return [member(text(1500 + 101 * i, 60 + i), LEVELS[(i + 2) % 4]) for i in range(12)]


def errors(target):
    ms = _twelve()
    st = starts_of(ms)
    good = b"".join(ms)
    ref, offs, _ = judge(good)
    assert len(offs) == 13
    cases = []
    m5 = bytearray(ms[5])                           # (level 9: Huffman data behind the 10-byte header)
    m5[10 + len(m5) // 3] ^= 0x10
    cases.append(("data", good[:st[5]] + bytes(m5) + good[st[6]:], 5, None))
    m5 = bytearray(ms[5]); m5[-8] ^= 0x01
    cases.append(("crc", good[:st[5]] + bytes(m5) + good[st[6]:], 5, (Z_DATA_ERROR, CHECK)))
    m5 = bytearray(ms[5]); m5[-4] ^= 0x01
    cases.append(("isize", good[:st[5]] + bytes(m5) + good[st[6]:], 5, (Z_DATA_ERROR, LENGTH)))
    cases.append(("cut in data", good[:st[11] + len(ms[11]) // 2], 11, (Z_BUF_ERROR, TRUNC)))
    cases.append(("cut in trailer", good[:len(good) - 3], 11, (Z_BUF_ERROR, TRUNC)))
    cases.append(("cut in the CRC", good[:len(good) - 6], 11, (Z_BUF_ERROR, TRUNC)))
    for name, data, idx, want in cases:
        if want is None:                            # what zlib makes of the damaged member with everything behind it
            k = zlib_case(data[st[idx]:])
            assert k in (DATA, CHECK, LENGTH, TRUNC)
            want = (Z_BUF_ERROR if k == TRUNC else Z_DATA_ERROR, k)
        cap = len(ref) + 1000
        r = target.raw(data, None, cap)
        assert r.rc == 0 and r.guard_ok, (name, r)
        assert (r.status, r.kind, r.index) == (want[0], want[1], idx), (name, r, want)
        assert r.members == idx and r.out_len == offs[idx] and r.in_used == st[idx], (name, r)
        assert r.out[:offs[idx]] == ref[:offs[idx]], name
        assert r.member_off[:idx + 1] == offs[:idx + 1], name
        try:
            target.all(data)
        except RuntimeError as e:
            assert "case %d" % want[1] in str(e), e
        else:
            raise AssertionError("no error raised for " + name)
    return len(cases)


# ---- 7. output capacity -----------------------------------------------------------------------------------------------------------
def capacity(target):
    data = b"".join(_twelve())
    ref, offs, covered = judge(data)
    r = target.raw(data, None, len(ref) - 1)
    assert r.rc == 0 and r.guard_ok, r
    assert (r.status, r.kind) == (Z_BUF_ERROR, OUT) and r.out_len == len(ref), r
    assert r.members == 11 and r.out[:offs[11]] == ref[:offs[11]]
    r = target.raw(data, None, 0)                   # no room at all: the call is the size query
    assert (r.status, r.kind, r.out_len, r.members) == (Z_BUF_ERROR, OUT, len(ref), 0) and r.guard_ok, r
    r = target.raw(data, None, len(ref))
    assert r.guard_ok
    expect_complete(r, ref, offs, covered)
    return 3


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------------
def arguments(target):
    """ZMI_E_ARG: as the return value where the host can see the mistake, in *d_status where only the device can (the list)"""
    ms = _twelve()[:4]
    data, st = b"".join(ms), starts_of(ms)
    r = target.raw(data, [], 10000)
    assert r.rc == E_ARG, r
    for lst in ([5] + st[1:], [st[0], st[2], st[1], st[3]], [st[0], st[1], st[1], st[2]], st + [len(data)]):
        r = target.raw(data, lst, 10000)
        assert r.rc == E_ARG or (r.rc == 0 and r.status == E_ARG and r.members == 0 and r.out_len == 0), (lst, r)
        assert r.guard_ok
    assert target.raw_null_result(data, st) == E_ARG
    r = target.raw(b"", [], 100)
    assert (r.rc, r.status, r.members, r.out_len, r.in_used) == (0, 0, 0, 0, 0), r
    r = target.raw(b"", [0], 100)
    assert (r.rc, r.status, r.members, r.out_len) == (0, 0, 0, 0), r
    return 7


# ---- the continuation loop (what Engine.inflate_members does; the emulator target runs it over raw()) ---------------------------------
def all_by_raw(target, data, starts=None):
    if starts is None:
        starts = target.find(data)
    ref_room = 4 * len(data) + (1 << 16)
    out, offs, pos, sub = b"", [], 0, list(starts)
    for _ in range(2 * len(starts) + 8):
        r = target.raw(data[pos:], sub, ref_room)
        if r.kind == OUT and r.out_len > ref_room:
            ref_room = r.out_len
            continue
        if r.rc != 0 or (r.status != 0 and r.kind != AGAIN):
            raise RuntimeError("status %d, case %d at proposal %d" % (r.status if r.rc == 0 else r.rc, r.kind, r.index))
        offs += [len(out) + o for o in r.member_off[:r.members]]
        out += r.out[:r.out_len]
        if r.status == 0:
            return out, offs + [len(out)]
        assert r.members >= 1
        pos += r.in_used
        sub = [0] + [s - pos for s in starts if s > pos]
    raise RuntimeError("no result")


# ---- a false proposal whose garbage ISIZE is possible but does not fit ----------------------------------------------------------------
def plausible_garbage(target):
    """a bogus start in Huffman data, placed where the four bytes in front of it read as a size deflate could reach from the bytes
    in front (so the plan cannot rule it out) but far above out_cap: still one call, with room to spare and with none"""
    plain = [member(text(900 + 13 * i, 40 + i), 6) for i in range(3)]
    big = member(text(150000, 14), 6)
    ms = plain[:1] + [big] + plain[1:]
    data, st = b"".join(ms), starts_of(ms)
    ref, offs, covered = judge(data)
    cands = [p for p in range(3000, len(big) - 100) if len(ref) + 8192 < struct.unpack("<I", big[p - 4:p])[0] <= 1032 * p]
    assert len(cands) >= 3
    for p in cands[:3]:
        lst = sorted(st + [st[1] + p])
        for room in (len(ref) + 4096, len(ref)):
            r = target.raw(data, lst, room)
            assert r.rc == 0 and r.guard_ok
            expect_complete(r, ref, offs, covered)
    return 3


# ---- members against the launch-group limit -------------------------------------------------------------------------------------
def group_limit_members(target, limit=256 << 10):
    """out_cap above the limit: a member above half the limit that shares its window overflows its group in the first pass and is
    decoded by the next one, which starts at it (still one call); one above the whole limit is ZMI_MM_BIG with Z_BUF_ERROR; the same
    files without the limit are one call"""
    mid = [member(text(n, 300 + i), 6) for i, n in enumerate([limit * 7 // 16, limit * 15 // 16, limit // 5])]
    big = [member(text(n, 310 + i), 6) for i, n in enumerate([limit // 4, limit * 3 // 2, limit // 8])]
    dm, db = b"".join(mid), b"".join(big)
    refm, offm, covm = judge(dm)
    refb, offb, covb = judge(db)
    expect_complete(target.raw(dm, None, len(refm) + 4096), refm, offm, covm)
    expect_complete(target.raw(db, None, len(refb) + 4096), refb, offb, covb)
    target.set_group_limit(limit)
    try:
        r = target.raw(dm, None, len(refm) + 4096)
        assert r.rc == 0 and r.guard_ok
        expect_complete(r, refm, offm, covm)
        expect_file(target, dm)
        r = target.raw(db, None, len(refb) + 4096)
        assert r.rc == 0 and r.guard_ok and (r.status, r.kind, r.index, r.members) == (Z_BUF_ERROR, BIG, 1, 1), r
        expect_prefix(r, db, refb, offb)
    finally:
        target.set_group_limit(None)
    return 2
