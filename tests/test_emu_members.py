"""CPU tests of the multi-member gzip calls on the emulator build (tests/emu/, -DZMI_EMU) with the checks of tests/members_checks.py --
the ones tests/test_gpu_members.py runs on the MI355X over the whole matrices.  The emulator runs a workgroup's threads as fibers:
here the bigger matrices run over the subsets named at each test; the GPU runs all of them."""
import ctypes as C

import os

import numpy as np
import pytest

import members_checks as K
import zmi_ctypes


class EmuTarget:
    def __init__(self):
        L = zmi_ctypes.load_emu()
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.zmi_gzip_find_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
        L.zmi_inflate_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
        self.L = L
        self.e = zmi_ctypes.Engine(L)
        self.ctx = self.e.ctx

    def close(self):
        self.e.close()

    def set_group_limit(self, nbytes):
        if nbytes is None:
            os.environ.pop("ZMI_MM_LIMIT", None)
        else:
            os.environ["ZMI_MM_LIMIT"] = str(int(nbytes))   # (read per call; the suite runs with ZMI_TUNING set)

    @staticmethod
    def _place(data, shift=0):
        raw = np.zeros(len(data) + 64, dtype=np.uint8)
        at = (shift - raw.ctypes.data) % 16
        buf = raw[at:at + len(data)]
        buf[:] = np.frombuffer(data, dtype=np.uint8)
        return raw, buf

    def find(self, data, cap=None, shift=0):
        keep, buf = self._place(data, shift)
        if cap is None:
            cap = len(data) // 18 + 1
        starts = np.full(cap + 1, 0x7777777777777777, dtype=np.uint64)
        cnt = np.full(1, 0x7777, dtype=np.uint32)
        rc = self.L.zmi_gzip_find_members_dev(self.ctx, buf.ctypes.data if len(data) else None, len(data), starts.ctypes.data, cap, cnt.ctypes.data, None)
        assert rc == 0
        assert int(cnt[0]) <= cap and int(starts[cap]) == 0x7777777777777777
        return [int(x) for x in starts[:int(cnt[0])]]

    def raw(self, data, starts, out_cap):
        if starts is None:
            starts = self.find(data)
        keep, buf = self._place(data, 3)
        st = np.array(list(starts) + [0], dtype=np.uint64)
        out = np.full(out_cap + K.GUARD, K.FILL, dtype=np.uint8)
        olen, used = np.full(1, 0x77, dtype=np.uint64), np.full(1, 0x77, dtype=np.uint64)
        members = np.full(1, 0x77, dtype=np.uint32)
        status, detail = np.full(1, 0x77, dtype=np.int32), np.full(1, 0x77, dtype=np.int32)
        moff = np.full(len(starts) + 2, 0x7777, dtype=np.uint64)
        rc = self.L.zmi_inflate_members_dev(self.ctx, buf.ctypes.data if len(data) else None, len(data), st.ctypes.data if len(starts) else None,
                                            len(starts), out.ctypes.data if out_cap else None, out_cap, olen.ctypes.data, used.ctypes.data,
                                            members.ctypes.data, moff.ctypes.data, status.ctypes.data, detail.ctypes.data, None)
        assert int(moff[len(starts) + 1]) == 0x7777
        return K.Result(rc, int(status[0]), int(detail[0]), int(members[0]), int(used[0]), int(olen[0]), bytes(out[:out_cap]),
                        bytes(out[out_cap:]) == bytes([K.FILL]) * K.GUARD, [int(x) for x in moff[:len(starts) + 1]])

    def raw_null_result(self, data, starts):
        keep, buf = self._place(data)
        st = np.array(starts, dtype=np.uint64)
        out = np.zeros(1 << 16, dtype=np.uint8)
        w = np.zeros(8, dtype=np.uint64)
        return self.L.zmi_inflate_members_dev(self.ctx, buf.ctypes.data, len(data), st.ctypes.data, len(starts), out.ctypes.data, out.size,
                                              w.ctypes.data, w.ctypes.data + 8, w.ctypes.data + 16, None, None, w.ctypes.data + 24, None)

    def all(self, data, starts=None):
        return K.all_by_raw(self, data, starts)

    def own_members(self, shards):
        out, st = self.e.deflate(shards, level=6, wrap=2)
        assert all(s == 0 for s in st)
        return out

    def pack(self, members):
        stride = (max(len(m) for m in members) + 31) & ~15
        return self.e.pack_slab(members, stride)


@pytest.fixture(scope="module")
def target():
    t = EmuTarget()
    yield t
    t.close()


def test_scan_is_exact(target):
    """all counts, lengths and levels (the scan alone is cheap on the emulator)"""
    assert K.scan_exactness(target) == 5


def test_boundary_straddles(target):
    """every offset around every boundary is searched; the files around 96 and 16384 are also decoded"""
    assert K.straddles(target, arounds=[1024, 4096], decode=False) == 22
    assert K.straddles(target, arounds=[96, 16384]) == 22


def test_header_fields(target):
    assert K.header_fields(target) == 64


def test_round_trip_of_own_output(target):
    """subset: 18 shards of 64 KiB; the 1 MiB limit gives 1.125 MiB / 512 KiB + 1 = 3 launch groups"""
    assert K.own_round_trip(target, n=18, shard=65536, low_limit=1 << 20) == 18


@pytest.mark.parametrize("case", list("abcde"))
def test_false_proposals(target, case):
    assert K.false_proposals(target, case) == {"a": 1, "b": 1, "c": 3, "d": 1, "e": 2}[case]


def test_false_proposal_with_possible_size(target):
    assert K.plausible_garbage(target) == 3


def test_members_against_the_group_limit(target):
    assert K.group_limit_members(target) == 2


def test_errors(target):
    assert K.errors(target) == 6


def test_output_capacity(target):
    assert K.capacity(target) == 3


def test_arguments(target):
    assert K.arguments(target) == 7
