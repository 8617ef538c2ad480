"""CPU tests of the checksum, combine, scan, stitch-plan, copy and frame kernels on the emulator build (tests/emu/, -DZMI_EMU),
with the checks of tests/checksum_pack_checks.py -- the ones tests/test_gpu_checksum_pack.py runs on the MI355X.  Under ZMI_EMU the
byte sums and the wave reduction of the checksum kernel are plain C, so what this file covers of that kernel is its indexing; it
also keeps the checks themselves and their host references tested without a GPU."""
import ctypes as C
import zlib

import numpy as np
import pytest

import checksum_pack_checks as K
import test_emu_stream_deflate as S
import zmi_ctypes


def _p(a):
    return a.ctypes.data if a is not None else None


def _aligned(a, align=256):
    """a copy of the byte array at an address that is a multiple of `align` (device allocations are; numpy's need not be)"""
    raw = np.empty(a.size + align, dtype=np.uint8)
    at = (-raw.ctypes.data) % align
    out = raw[at:at + a.size]
    out[:] = a.reshape(-1)
    assert out.ctypes.data % align == 0
    return out


class EmuTarget:
    def __init__(self):
        self.L = S._bind(zmi_ctypes.load_emu())
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        self.L.zmi_checksum_batch_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp]
        self.L.zmi_scan_sizes_dev.argtypes = [vp, vp, u32, vp, vp]
        self.e = S._Ctx(self.L)
        self.ctx, self.ok = self.e.ctx, self.e.ok

    def close(self):
        self.e.close()

    def checksums(self, buf, launches):
        b = _aligned(buf)
        res = []
        for off, lens, kind, a0, c0 in launches:
            a, c = a0.copy(), c0.copy()
            self.ok(self.L.zmi_checksum_batch_dev(self.ctx, _p(b), _p(off), _p(lens), len(lens), kind, _p(a), _p(c), None), "checksums")
            res.append((a, c))
        return b.ctypes.data, res

    def combine(self, checks, lens, wrap, world):
        oc, ol = np.full(1, 9, dtype=np.uint32), np.full(1, 9, dtype=np.uint64)
        n = len(lens)
        self.ok(self.L.zmi_checksum_combine_dev(self.ctx, wrap, _p(checks) if n else None, _p(lens) if n else None, world, n // world,
                                                _p(oc), _p(ol), None), "combine")
        return int(oc[0]), int(ol[0])

    def scan_sizes(self, lens):
        off = np.full(len(lens) + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        self.ok(self.L.zmi_scan_sizes_dev(self.ctx, _p(lens) if len(lens) else None, len(lens), _p(off), None), "scan")
        return off

    def stitch_plan(self, table):
        world, n_local = table.shape
        table = np.ascontiguousarray(table)
        goff = np.zeros((world, n_local), dtype=np.uint64)
        soff = np.zeros((world, n_local + 1), dtype=np.uint64)
        d_tot, host = np.zeros(world + 1, dtype=np.uint64), np.zeros(world + 1, dtype=np.uint64)
        self.ok(self.L.zmi_stitch_plan_dev(self.ctx, _p(table), world, n_local, _p(goff), _p(soff), _p(d_tot), _p(host), None), "plan")
        assert np.array_equal(d_tot, host)
        return goff, soff, [int(x) for x in host]

    def copy_ranges(self, src, src_off, src_stride, lens, max_len, dst, dst_off, dst_cap):
        s, d = _aligned(src), _aligned(dst)
        self.ok(self.L.zmi_copy_ranges_dev(self.ctx, _p(s), _p(src_off), src_stride, _p(lens), len(lens), max_len, _p(d), _p(dst_off),
                                           dst_cap, None), "copy")
        return s.ctypes.data, d.ctypes.data, d

    def pack_slab(self, slots, lens, slab):
        s, d = _aligned(slots), _aligned(slab)
        off = np.zeros(len(lens) + 1, dtype=np.uint64)
        self.ok(self.L.zmi_pack_slab_dev(self.ctx, _p(s), slots.shape[1], _p(lens), len(lens), _p(d), d.size, _p(off), None), "pack")
        return s.ctypes.data, d, off

    def frame(self, out, cap, payload_len, check, raw_len, wrap, level, strategy):
        pl, ck, rl = np.array([payload_len], np.uint64), np.array([check], np.uint32), np.array([raw_len], np.uint64)
        olen, st = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.int32)
        self.ok(self.L.zmi_stream_frame_dev(self.ctx, wrap, level, strategy, _p(pl), _p(ck), _p(rl), _p(out), cap, _p(olen), _p(st), None),
                "frame")
        return out, int(olen[0]), int(st[0])


@pytest.fixture(scope="module")
def target():
    t = EmuTarget()
    yield t
    t.close()


# ---- the host references themselves --------------------------------------------------------------------------------------
def test_reference_combines_against_zlib():
    """the pure-Python crc32_combine / adler32_combine against zlib.crc32 / zlib.adler32 of real concatenations, against the system
    zlib's combine functions for lengths up to 2^32 - 1 where that library loads, and the vector fold against the scalar one"""
    rng = np.random.default_rng(1)
    lengths = [0, 1, 65520, 65521, 65522] + [int(x) for x in rng.integers(2, 1 << 20, 4)]
    blobs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths] + [b"\xff" * 70000, bytes(65521)]
    for a in blobs:
        for b in blobs:
            assert K.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b), (len(a), len(b))
            assert K.adler32_combine(zlib.adler32(a), zlib.adler32(b), len(b)) == zlib.adler32(a + b), (len(a), len(b))
    pieces = blobs[:7]
    whole = b"".join(pieces)
    assert K.fold_scalar([zlib.crc32(p) for p in pieces], [len(p) for p in pieces], 2) == (zlib.crc32(whole), len(whole))
    assert K.fold_scalar([zlib.adler32(p) for p in pieces], [len(p) for p in pieces], 1) == (zlib.adler32(whole), len(whole))
    assert K.fold_crc_vector([zlib.crc32(p) for p in pieces], [len(p) for p in pieces]) == (zlib.crc32(whole), len(whole))
    for n, pattern in ((1, "random"), (2, "max"), (77, "pow2"), (301, "random"), (500, "max"), (400, "adler_edges"), (3, "zero")):
        lens = K._combine_lens(pattern, n, rng)
        checks = K._combine_checks(n, 2)
        assert K.fold_crc_vector(checks, lens) == K.fold_scalar(checks, lens, 2), (n, pattern)
    try:
        sysz = C.CDLL("libz.so.1")
    except OSError:
        return                      # (only this part needs the system library)
    for f in (sysz.crc32_combine64, sysz.adler32_combine64):
        f.restype = C.c_ulong
        f.argtypes = [C.c_ulong, C.c_ulong, C.c_int64]
    lens = [1, 2, 65520, 65521, 65522, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFF - 65521] + [int(x) for x in rng.integers(1, 1 << 32, 40)]
    for i, l in enumerate(lens):
        c1, c2 = (int(x) for x in rng.integers(0, 1 << 32, 2))
        assert K.crc32_combine(c1, c2, l) == sysz.crc32_combine64(c1, c2, l), l
        halves = [0, 65520, 1, int(rng.integers(0, K.BASE))]
        a1 = (halves[i % 4] << 16) | halves[(i // 4) % 4]
        a2 = (int(rng.integers(0, K.BASE)) << 16) | halves[(i + 1) % 4]
        assert K.adler32_combine(a1, a2, l) == sysz.adler32_combine64(a1, a2, l), (hex(a1), hex(a2), l)


def test_reference_header_and_trailer_bytes():
    assert K.header_bytes(1, 6, 0) == b"\x78\x9c" and K.header_bytes(1, 9, 0) == b"\x78\xda" and K.header_bytes(1, 9, 2) == b"\x78\x01"
    assert K.header_bytes(2, 6, 0) == b"\x1f\x8b\x08\0\0\0\0\0\0\x03" and K.header_bytes(2, 9, 0)[8] == 2 and K.header_bytes(2, 1, 0)[8] == 4
    assert K.header_bytes(0, 6, 0) == b""
    data = b"frame me" * 100
    for wrap, wbits in ((1, 15), (2, 31)):
        co = zlib.compressobj(6, zlib.DEFLATED, wbits)
        s = co.compress(data) + co.flush()
        check = zlib.adler32(data) if wrap == 1 else zlib.crc32(data)
        assert s.startswith(K.header_bytes(wrap, 6, 0)) and s.endswith(K.trailer_bytes(wrap, check, len(data)))
    assert K.trailer_bytes(2, 1, (1 << 32) + 5) == b"\x01\0\0\0\x05\0\0\0"


# ---- 1. checksum kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", K.CHECKSUM_CONTENTS)
def test_checksum_length_residue_matrix(target, content):
    assert K.checksum_matrix(target, content) == 40 * 16 * 3


def test_checksum_one_shard_and_many_ragged_shards(target):
    assert K.checksum_fixed_launches(target) == 3501


def test_checksum_4mib_of_ff_aligned_and_at_residue_3(target):
    """(64 MiB on the GPU)"""
    assert K.checksum_large_ff(target, n=(4 << 20) + 5) == 2


# ---- 2. combine kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", K.COMBINE_WORLDS)
@pytest.mark.parametrize("wrap", [1, 2])
def test_combine_matrix(target, wrap, world):
    assert K.combine_matrix(target, wrap, world) == 14 * 7 + 1


@pytest.mark.parametrize("world", [1, 3])
def test_combine_of_piece_checksums_is_the_checksum_of_the_buffer(target, world):
    K.combine_end_to_end(target, world)


# ---- 3. scan and stitch plan ---------------------------------------------------------------------------------------------
def test_scan_sizes(target):
    assert K.scan_checks(target) == 24


def test_stitch_plan(target):
    assert K.stitch_plan_checks(target) == 16


# ---- 4. copy kernel ------------------------------------------------------------------------------------------------------
def test_copy_every_length_and_alignment_one_workgroup_per_range(target):
    assert K.copy_many_ranges(target) == 23 * 256


def test_copy_few_large_ranges_share_workgroups(target):
    assert K.copy_few_large_ranges(target) == 16 + 11 + 11


def test_copy_skips_a_range_behind_the_capacity(target):
    assert K.copy_capacity(target) == 25


def test_pack_slab_from_odd_strides(target):
    assert K.pack_slab_checks(target) == 360


# ---- 5. frame kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [0, 1, 2])
def test_frame_header_trailer_and_guard_bytes(target, wrap):
    assert K.frame_checks(target, wrap) == (408 if wrap == 0 else 462)   # (an empty raw stream has no capacity below it)
