"""The multi-member gzip calls on the MI355X through Engine (find_members / inflate_members), with the checks of
tests/members_checks.py over their whole matrices; zlib / gzip on the CPU judge."""
import os
import zlib

import numpy as np
import pytest
import torch

import members_checks as K

pytestmark = pytest.mark.gpu


class GpuTarget:
    def __init__(self):
        from zlib_rs_amd.engine import Engine
        self.e = Engine(0)
        self.dev = self.e.device

    def close(self):
        self.e.close()

    def set_group_limit(self, nbytes):
        if nbytes is None:
            os.environ.pop("ZMI_MM_LIMIT", None)
        else:
            os.environ["ZMI_MM_LIMIT"] = str(int(nbytes))   # (read per call; the suite runs with ZMI_TUNING set)

    def _dev(self, data, shift=0):
        """the bytes on the device, `shift` bytes behind a 16-byte boundary"""
        buf = torch.zeros(len(data) + 32, dtype=torch.uint8, device=self.dev)
        at = (shift - buf.data_ptr()) % 16
        view = buf[at:at + len(data)]
        if data:
            view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        return view

    def find(self, data, cap=None, shift=0):
        return self.e.find_members(self._dev(data, shift), cap).tolist()

    def raw(self, data, starts, out_cap):
        d = self._dev(data, 3)
        s = self.e.find_members(d) if starts is None else torch.tensor(list(starts), dtype=torch.int64, device=self.dev)
        room = torch.full((out_cap + K.GUARD,), K.FILL, dtype=torch.uint8, device=self.dev)
        moff = torch.full((int(s.numel()) + 2,), 0x7777, dtype=torch.int64, device=self.dev)
        try:
            st, kind, idx, members, used, olen = self.e.inflate_members_raw(d, s, room[:out_cap], moff)
        except RuntimeError as err:
            assert "rc=-103" in str(err), err
            return K.Result(K.E_ARG, 0, 0, 0, 0, 0, b"", True, [])
        host = room.cpu().numpy().tobytes()
        m = moff.tolist()
        assert m[-1] == 0x7777
        return K.Result(0, st, kind | (idx << 8), members, used, olen, host[:out_cap], host[out_cap:] == bytes([K.FILL]) * K.GUARD, m[:-1])

    def raw_null_result(self, data, starts):
        d = self._dev(data)
        s = torch.tensor(list(starts), dtype=torch.int64, device=self.dev)
        out = torch.zeros(1 << 16, dtype=torch.uint8, device=self.dev)
        w = torch.zeros(4, dtype=torch.int64, device=self.dev)
        return self.e.L.zmi_inflate_members_dev(self.e._ctx, d.data_ptr(), len(data), s.data_ptr(), len(starts), out.data_ptr(), out.numel(),
                                                w.data_ptr(), w.data_ptr() + 8, w.data_ptr() + 16, None, None, w.data_ptr() + 24, None)

    def all(self, data, starts=None):
        s = None if starts is None else torch.tensor(list(starts), dtype=torch.int64, device=self.dev)
        out, moff = self.e.inflate_members(self._dev(data, 3), s, index=True)
        return out.cpu().numpy().tobytes(), moff.tolist()

    def _deflate(self, shards):
        from zlib_rs_amd.engine import WRAP_GZIP
        lens = [len(s) for s in shards]
        off = np.zeros(len(shards), dtype=np.int64)
        off[1:] = np.cumsum(lens[:-1])
        data = self._dev(b"".join(shards) + b"\0")
        out, olen, st = self.e.deflate_batch(data, torch.from_numpy(off).to(self.dev), torch.tensor(lens, dtype=torch.int32, device=self.dev),
                                             max(lens), level=6, wrap=WRAP_GZIP)
        assert (st.cpu().numpy() == 0).all()
        return out, olen

    def own_members(self, shards):
        out, olen = self._deflate(shards)
        host, ln = out.cpu().numpy(), olen.cpu().numpy()
        return [host[i, :ln[i]].tobytes() for i in range(len(shards))]

    def pack(self, members):
        stride = (max(len(m) for m in members) + 31) & ~15
        slots = torch.zeros((len(members), stride), dtype=torch.uint8, device=self.dev)
        host = np.zeros((len(members), stride), dtype=np.uint8)
        for i, m in enumerate(members):
            host[i, :len(m)] = np.frombuffer(m, dtype=np.uint8)
        slots.copy_(torch.from_numpy(host))
        slab, off = self.e.pack_slab(slots, torch.tensor([len(m) for m in members], dtype=torch.int32, device=self.dev))
        off = off.tolist()
        return slab[:off[-1]].cpu().numpy().tobytes(), off


@pytest.fixture(scope="module")
def target():
    t = GpuTarget()
    yield t
    t.close()


def test_scan_is_exact(target):
    assert K.scan_exactness(target) == 5


def test_scan_files_decode(target):
    """the files of the scan test (1, 2, 3 and 300 members, every length and level, the library's own members) also decode"""
    for data in K.scan_files(target):
        K.expect_file(target, data)


def test_boundary_straddles(target):
    assert K.straddles(target) == 44


def test_header_fields(target):
    assert K.header_fields(target) == 64


def test_round_trip_of_own_output(target):
    """64 shards of 64 KiB; the 1 MiB limit gives 4 MiB / 512 KiB + 1 = 9 launch groups"""
    assert K.own_round_trip(target, n=64, shard=65536, low_limit=1 << 20) == 64


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


def test_independent_of_earlier_inflate_calls(target):
    """Engine.inflate_batch leaves the context's inflate-out limit sized for its own small call; a file with a member of a few MiB
    decodes afterwards as it does on a fresh context, in one call, and a list that ends early does not end the file"""
    from zlib_rs_amd.engine import WRAP_ZLIB
    e, dev = target.e, target.dev
    small = zlib.compress(K.text(3000, 1))
    src = target._dev(small)
    out = torch.zeros(4096, dtype=torch.uint8, device=dev)
    z = torch.zeros(1, dtype=torch.int64, device=dev)
    blen, bst = e.inflate_batch(src, z, torch.tensor([len(small)], dtype=torch.int32, device=dev), out, z.clone(),
                                torch.tensor([4096], dtype=torch.int32, device=dev), wrap=WRAP_ZLIB)
    assert bst.tolist() == [0] and out[:3000].cpu().numpy().tobytes() == K.text(3000, 1)
    ms = [K.member(K.text(n, 400 + i), 6) for i, n in enumerate([5000, 3 << 20, 70000])]
    data = b"".join(ms)
    ref, offs, covered = K.judge(data)
    r = target.raw(data, None, 4 * len(data) + (1 << 20))
    K.expect_complete(r, ref, offs, covered)
    got, moff = target.all(data)
    assert got == ref and moff == offs
    got, moff = target.all(data, K.starts_of(ms)[:2])     # the caller's list misses the last start
    assert got == ref and moff == offs and e.last_members_in_used == len(data)
    got, moff = target.all(data + b"trailing bytes")
    assert got == ref and e.last_members_in_used == len(data)
