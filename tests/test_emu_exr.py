"""CPU tests of the OpenEXR reader (zmi_exr_headers_dev / zmi_exr_read_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the
checks of tests/exr_checks.py -- the ones tests/test_gpu_exr.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import pytest

import exr_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def test_geometry(target):
    """widths 1, 3, 17, 64, 65 and 257, heights 1, 16, 17 and 33, every compression and channel layout (the GPU test adds widths 2, 5
    and 63 and height 15)"""
    assert K.geometry(target, widths=(1, 3, 17, 64, 65, 257), heights=(1, 16, 17, 33)) == 3 * 3 * 6 * 4


def test_trips(target):
    """ZIP only (the GPU test adds ZIPS)"""
    assert K.trips(target, comps=(K.ZIP,)) == 10


def test_carries(target):
    """a chunk of 4 x 4099 RGBA HALF: 129 blocks, every run a whole piece and a second of 6 bytes (the GPU test: 16 rows, 524 KiB)"""
    assert K.carries(target, rows=4) == 1


def test_raw_chunks(target):
    assert K.raw_chunks(target) == 4


def test_tiles(target):
    assert K.tiles(target) == 12


def test_layout(target):
    assert K.layout(target) == 22


def test_statuses(target):
    assert K.statuses(target) == 40 + 26


def test_selection_and_room(target):
    assert K.selection(target) == 10 + 4 + 5


def test_forged_record(target):
    assert K.forged_record(target) == 24


def test_independence(target, inf_selection):
    """eight files (the GPU test: twelve)"""
    assert K.independence(target, count=8) == 9


def test_arguments(target):
    assert K.arguments(target) == 11
