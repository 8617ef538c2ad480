"""CPU tests of the PNG reader (zmi_png_headers_dev / zmi_png_decode_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the checks
of tests/png_checks.py -- the ones tests/test_gpu_png.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import pytest

import png_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def test_geometry(target):
    """heights 1, 64, 65 and 129 against widths 1, 63 and 65 (the GPU test adds height 63 and width 64), and every strip case"""
    assert K.geometry(target, heights=(1, 64, 65, 129), widths=(1, 63, 65)) == 2 * 12 + 8 + 3 + 3 + 3


def test_formats(target):
    assert K.formats(target) == 30


def test_filters(target):
    assert K.filters(target) == 10 + 25 + 6 + 3 + 5


def test_idat_layout(target):
    """the file of many IDAT chunks has 60 of them (the GPU test: 300)"""
    assert K.idat_layout(target, many=60) == 14


@pytest.mark.parametrize("count", [1, 3, 64, 65, 300])
def test_batches(target, count):
    """1, 3 and 65 images at the four input alignments with the output alignments 1, 16 and 4096 in turn; 64 images at two alignments,
    300 at one"""
    shifts = K.SHIFTS if count in (1, 3, 65) else ([3, 15] if count == 64 else [15])
    assert K.batches(target, counts=[count], shifts=shifts) == len(shifts)


def test_selection_and_room(target):
    assert K.selection(target) == 14


def test_statuses(target):
    assert K.statuses(target) == 38


def test_no_crc(target):
    assert K.no_crc(target) == 38


def test_scratch_limit_status(target):
    assert K.scratch(target) == 3


def test_forged_record(target):
    assert K.forged_record(target) == 3


def test_determinism(target):
    assert K.determinism(target) == 9


def test_arguments(target):
    assert K.arguments(target) == 10
