"""CPU tests of the ZIP reader (zmi_zip_directory_dev / zmi_zip_inflate_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the
checks of tests/zip_checks.py -- the ones tests/test_gpu_zip.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import numpy as np
import pytest

import zip_checks as K
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


def test_small_shapes(target):
    assert K.small_shapes(target) == 6


@pytest.mark.parametrize("count", [3, 64, 65, 300])
def test_shapes(target, count):
    """3 and 65 entries at the four input alignments with the output alignments 1, 16 and 4096 in turn; 64 entries at two alignments, 300
    at one, with output alignment 16"""
    if count in (3, 65):
        assert K.shapes(target, counts=[count]) == 4
    else:
        shifts = [3, 15] if count == 64 else [15]
        assert K.shapes(target, counts=[count], shifts=shifts, aligns=(16,)) == len(shifts)


def test_end_record(target):
    assert K.end_record(target) == 10


def test_chain_across_window_edges(target):
    """the second entry 0, 1, 3, 4 and 45 bytes in front of the window's end, and the entry of 46 + 3 x 65 535 bytes"""
    assert K.chain_edges(target, ss=[0, 1, 3, 4, 45]) == 10
    assert K.long_entry(target) == 1


def test_chain_where_the_signature_misleads(target):
    assert K.false_guesses(target) == 9


def test_directory_sizes(target):
    assert K.directory_sizes(target) == 3


def test_zip64(target):
    assert K.zip64_extras(target) == 12


def test_local_header_differs(target):
    assert K.local_differs(target) == 4


def test_flagged_entries(target):
    assert K.flagged(target) == 13


def test_corruption(target):
    assert K.corruption(target) == 9


def test_archive_errors(target):
    assert K.archive_errors(target) == 6


def test_selection_and_room(target):
    assert K.selection(target) == 16


def test_arguments(target):
    assert K.arguments(target) == 8


def test_determinism(target):
    assert K.determinism(target) == 5
