"""GPU tests (-m gpu) of the checksum, combine, scan, stitch-plan, copy and frame kernels through zlib_rs_amd.engine.Engine, with
the checks of tests/checksum_pack_checks.py: exact equality against plain host references.  Here the checksum kernel runs as it
ships -- v_sad_u8 / v_dot4_u32_u8 byte sums, the DPP wave reduction -- at every start residue, which the emulator build replaces
with plain C and the other GPU tests never leave 16-byte alignment for; `world > 1` is table layout only, in one process."""
import numpy as np
import pytest

import checksum_pack_checks as K

pytestmark = pytest.mark.gpu


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class GpuTarget:
    def __init__(self, engine):
        import torch
        self.torch, self.e = torch, engine

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.e.device)

    def checksums(self, buf, launches):
        d = self.dev(buf)
        res = []
        for off, lens, kind, a0, c0 in launches:
            a, c = self.dev(_i32(a0)), self.dev(_i32(c0))
            self.e.checksums(d, self.dev(_i64(off)), self.dev(_i32(lens)), adler=bool(kind & 1), crc=bool(kind & 2), out_adler=a, out_crc=c)
            res.append((_u32(a), _u32(c)))
        return d.data_ptr(), res

    def combine(self, checks, lens, wrap, world):
        c, t = self.e.checksum_combine(self.dev(_i32(checks)), self.dev(_i32(lens)), wrap=wrap, world=world)
        return int(_u32(c)[0]), int(_u64(t)[0])

    def scan_sizes(self, lens):
        out = self.torch.full((len(lens) + 1,), 0x5A5A5A5A5A5A5A5A, dtype=self.torch.int64, device=self.e.device)
        return _u64(self.e.scan_sizes(self.dev(_i32(lens)), out=out))

    def stitch_plan(self, table):
        goff, soff, totals = self.e.stitch_plan(self.dev(_i32(table)))
        return _u64(goff), _u64(soff), totals

    def copy_ranges(self, src, src_off, src_stride, lens, max_len, dst, dst_off, dst_cap):
        s, d = self.dev(src), self.dev(dst)
        self.e.copy_ranges(s, self.dev(_i64(src_off)) if src_off is not None else None, src_stride, self.dev(_i32(lens)), max_len,
                           d[:dst_cap], self.dev(_i64(dst_off)))
        return s.data_ptr(), d.data_ptr(), d.cpu().numpy()

    def pack_slab(self, slots, lens, slab):
        s, d = self.dev(slots), self.dev(slab)
        _, off = self.e.pack_slab(s, self.dev(_i32(lens)), slab=d)
        return s.data_ptr(), d.cpu().numpy(), _u64(off)

    def frame(self, out, cap, payload_len, check, raw_len, wrap, level, strategy):
        d = self.dev(out)
        meta = self.e.stream_frame(d, self.dev(_i64([payload_len])), self.dev(_i32([check])), self.dev(_i64([raw_len])), wrap=wrap,
                                   level=level, strategy=strategy, out_cap=cap)
        length, st = meta.tolist()
        st &= 0xFFFFFFFF
        return d.cpu().numpy(), int(length), st - (1 << 32) if st >= 1 << 31 else st


@pytest.fixture(scope="module")
def target(engine):
    return GpuTarget(engine)


# ---- 1. checksum kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", K.CHECKSUM_CONTENTS)
def test_checksum_length_residue_matrix(target, content):
    """40 lengths x 16 start residues x 3 kinds per kind of contents: 26 MiB of input, three launches"""
    assert K.checksum_matrix(target, content) == 40 * 16 * 3


def test_checksum_one_shard_and_many_ragged_shards(target):
    assert K.checksum_fixed_launches(target) == 3501


def test_checksum_64mib_of_ff_aligned_and_at_residue_3(target):
    assert K.checksum_large_ff(target) == 2


# ---- 2. combine kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", K.COMBINE_WORLDS)
@pytest.mark.parametrize("wrap", [1, 2])
def test_combine_matrix(target, wrap, world):
    """15 entry counts x 7 kinds of lengths; rank-major tables with padded short ranks for world > 1"""
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
