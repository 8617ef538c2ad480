"""CPU tests of zmi_inflate_sizes_dev / zmi_inflate_batch_packed_dev on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/inflate_sizes_checks.py -- the ones tests/test_gpu_inflate_sizes.py runs on the MI355X over the whole matrices.  The emulator
runs a workgroup's threads as fibers: the length x mode matrix runs here without its two largest lengths (in every mode but the
special streams, which keep their sizes); the GPU runs all of it."""
import numpy as np
import pytest

import inflate_sizes_checks as K
import zmi_ctypes

SMALL = tuple(K.SMALL_LENS)


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


class EmuTarget(K.AbiTarget):
    def __init__(self):
        self.e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
        super().__init__(self.e.lib, self.e.ctx, HostMem())

    def close(self):
        self.e.close()

    def own(self, shards, level, wrap):
        out, st = self.e.deflate(list(shards), level=level, wrap=wrap)
        assert all(s == 0 for s in st)
        return out


@pytest.fixture(scope="module")
def target():
    t = EmuTarget()
    yield t
    t.close()


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_sizes_are_exact(target, inf_selection, wrap):
    assert K.sizes_exact(target, wrap, SMALL) == 7 * len(SMALL) + 9


def test_sizes_of_the_largest_lengths(target, inf_selection):
    """300 000 and 1 MiB + 1 bytes at level 6 and stored, which the matrix above leaves out"""
    raws = [K.text(n, 1234) for n in K.LENS[-2:]]
    streams = [K.deflate(r, K.ZLIB, level) for r in raws for level in (6, 0)]
    got = target.sizes(streams, K.ZLIB)
    assert [w.key() for w in got] == [(len(r), 0, len(s), 0) for r, s in zip([raws[0]] * 2 + [raws[1]] * 2, streams)]


def test_sizes_of_many_tiny_streams(target, inf_selection):
    assert K.sizes_many_tiny(target) == 600


def test_sizes_of_own_output(target, inf_selection):
    assert K.sizes_own_output(target, lens=(0, 1, 4097, 70000)) == 36


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_independence(target, inf_selection, wrap):
    assert K.independence(target, wrap) >= 25


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_failing_streams(target, inf_selection, wrap):
    assert K.failing_streams(target, wrap) >= 9


def test_history(target, inf_selection):
    assert K.history(target) == 5


def test_wrong_check_values(target, inf_selection):
    assert K.wrong_checks(target) == 3


def test_size_limit(target, inf_selection):
    assert K.size_limit(target) == 7


@pytest.mark.parametrize("align", [1, 16, 4096])
def test_packed_equals_batch(target, inf_selection, align):
    """zlib at every alignment, the other wrappers at 16 over five of the lengths"""
    assert K.packed_equals_batch(target, K.ZLIB, align, SMALL) == 7 * len(SMALL) + 9
    if align == 16:
        for wrap in (K.RAW, K.GZIP, K.AUTO):
            K.packed_equals_batch(target, wrap, align, (0, 1, 259, 4097, 65537))


def test_packed_with_a_shared_dictionary(target, inf_selection):
    assert K.packed_shared_dict(target) == 13


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(target, inf_selection, align):
    assert K.capacity(target, align=align) == 4


def test_arguments(target):
    assert K.arguments(target) == 17


def test_context_limit_is_the_callers(target):
    """... also across the host-buffer batch and the single-stream call, which size their own scratch too (twelve streams: both decode
    selections are the same kernel)"""
    def host_calls(streams, raws):
        out, st = target.e.inflate(streams, [len(r) for r in raws], wrap=K.ZLIB)
        assert st == [0] * len(raws) and out == raws
        got, status, _, used, res = target.e.inflate_resume(streams[0][2:-4], cap=len(raws[0]) + 64)
        assert (got, status, used, res[3]) == (raws[0], 0, len(streams[0]) - 6, 1)

    assert K.context_limit(target, between=host_calls) == 4
