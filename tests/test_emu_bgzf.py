"""CPU tests of the BGZF writer (zmi_bgzf_blocks_dev / zmi_bgzf_deflate_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the
checks of tests/bgzf_checks.py -- the ones tests/test_gpu_bgzf.py runs on the MI355X over the whole matrices.  The emulator runs a
workgroup's threads as fibers, so the shape matrix is thinned here to the subsets named at each test; the other checks run whole.
BgzfIndex's host side (.gzi files, virtual offsets) needs no device and is checked here against the walker."""
import os
import struct

import numpy as np
import pytest

import bgzf_checks as K
import zmi_ctypes


class HostMem:
    """the emulator's device memory is host memory"""
    stream = None

    class Handle:
        def __init__(self, keep, view):
            self.keep, self.view, self.ptr = keep, view, view.ctypes.data

    def put(self, arr, shift=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        raw = np.zeros(b.size + 32, dtype=np.uint8)
        at = (shift - raw.ctypes.data) % 16
        view = raw[at:at + b.size]
        view[:] = b
        return self.Handle(raw, view)

    def full(self, nbytes, fill):
        return self.put(np.full(nbytes, fill, dtype=np.uint8))

    def read(self, h, dtype):
        return h.view.copy().view(dtype)


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def test_small_shapes(target):
    """every level and strategy, kind and alignment at the sizes 0, 1 and 5 with block sizes 65280, 777 and 1"""
    assert K.shapes(target, ns=[0, 1, 5], bbs=[65280, 777, 1]) == 3 * 3 * 4 * 6 * 4


@pytest.mark.parametrize("n,shifts", [(65279, [0, 1, 3, 15]), (65280, [0, 1, 3, 15]), (65281, [0, 1, 3, 15]), (3 * 65280 + 17, [0, 15])])
def test_sizes_around_the_block_limit(target, n, shifts):
    """the alternation of text, zeros and random bytes at level 6, blocks of 65280 at the four alignments (the largest size at two) and of
    4096 and 777 at one"""
    assert K.shapes(target, configs=[(6, 0)], kinds=["mix"], ns=[n], bbs=[65280], shifts=shifts) == len(shifts)
    assert K.shapes(target, configs=[(6, 0)], kinds=["mix"], ns=[n], bbs=[4096, 777], shifts=[3]) == 2


@pytest.mark.parametrize("config", [(0, 0), (1, 0), (9, 0), (6, 2), (6, 3)])
def test_levels_and_strategies_on_two_blocks(target, config):
    """2 x 65280 bytes of every kind under the other levels and strategies, at one alignment"""
    assert K.shapes(target, configs=[config], ns=[2 * 65280], bbs=[65280], shifts=[1]) == 4


def test_limit_and_fallback(target):
    """blocks of 4096 under every level and strategy, blocks of 65280 at level 6"""
    assert K.fallback(target, bbs=[4096]) == 6 * 6
    assert K.fallback(target, configs=[(6, 0)], bbs=[65280], blocks=3) == 3


def test_index_is_optional(target):
    assert K.index_optional(target) == 2


def test_grouping(target):
    assert K.grouping(target, _setenv) == 10


def test_empty_shards(target):
    assert K.empty_shards(target) == 4


def test_capacity(target):
    assert K.capacity(target) == 9


def test_arguments(target):
    assert K.arguments(target) == 21 + 3


def test_own_readers(target):
    assert K.own_readers(target) == 2


# ---- BgzfIndex on the host ------------------------------------------------------------------------------------------------------------------
def _index_of(target, data, bb):
    import torch
    from zlib_rs_amd.engine import BgzfIndex
    res = target.deflate(data, bb)
    offs, _ = K.check_file(res, data, bb)
    return res.file, offs, BgzfIndex(torch.tensor(res.off, dtype=torch.int64), bb, len(data))


def test_gzi_files_and_virtual_offsets(target, tmp_path):
    from zlib_rs_amd.engine import BgzfIndex
    bb = 777
    data = K.make("mix", 7 * bb + 5, bb)
    file, offs, index = _index_of(target, data, bb)
    assert index.n_blocks == 8
    path = str(tmp_path / "a.gzi")
    index.save_gzi(path)
    want = struct.pack("<Q", 7) + b"".join(struct.pack("<QQ", offs[i], i * bb) for i in range(1, 8))
    assert open(path, "rb").read() == want
    back = BgzfIndex.load_gzi(path, file, "cpu")
    assert (back.block_bytes, back.n, back.block_off.tolist()) == (bb, len(data), offs)
    for u in (0, 1, bb - 1, bb, 3 * bb + 7, len(data) - 1, len(data)):
        assert index.virtual_offset(u) == offs[u // bb] << 16 | u % bb == back.virtual_offset(u)
    sx = index.stream_index()
    assert sx.win is None and sx.max_gap == bb and sx.bit.tolist() == [8 * (o + 18) for o in offs[:8]]
    assert sx.out.tolist() == [i * bb for i in range(8)] + [len(data)]


def test_gzi_of_files_with_one_block_and_none(target, tmp_path):
    from zlib_rs_amd.engine import BgzfIndex
    for n in (0, 300):
        data = K.make("text", n, 4096)
        file, offs, index = _index_of(target, data, 4096)
        path = str(tmp_path / ("%d.gzi" % n))
        index.save_gzi(path)
        assert open(path, "rb").read() == struct.pack("<Q", 0)
        with pytest.raises(ValueError):
            BgzfIndex.load_gzi(path, file, "cpu")                   # block_bytes is not in the table
        back = BgzfIndex.load_gzi(path, file, "cpu", block_bytes=4096)
        assert (back.block_bytes, back.n, back.block_off.tolist()) == (4096, n, offs)
        assert back.stream_index().max_gap == min(4096, n)
