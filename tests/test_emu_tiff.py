"""CPU tests of the TIFF reader (zmi_tiff_directory_dev / zmi_tiff_read_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the
checks of tests/tiff_checks.py -- the ones tests/test_gpu_tiff.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import pytest

import tiff_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def test_geometry(target):
    """tiles of 16 x 16 only (the GPU test adds 16 x 32); every strip case; row bytes around the row tile in pixels of 1, 3 and 8 bytes
    (the GPU test adds 4 and 6)"""
    assert K.geometry(target, tiles=((16, 16),), pixels=((1, 8), (3, 8), (1, 64))) == 5 + 9 + 3 * 4


def test_formats(target):
    """depths 8, 16 and 64, 1 and 3 samples, both byte orders (the GPU test adds depth 32 and 2 and 4 samples); the five pages of 5, 7
    and 8 samples"""
    assert K.formats(target, depths=(8, 16, 64), sample_counts=(1, 3)) == 8 + 12 + 12 + 5


def test_layout(target):
    assert K.layout(target) == 12 + 4 + 1 + 1


def test_selection_and_room(target):
    assert K.selection(target) == 4 * 16 + 3 + 3 + 2 + 2


def test_statuses(target):
    assert K.statuses(target) == 10 + 24 + 6


def test_forged_record(target):
    assert K.forged_record(target) == 14


def test_determinism(target, inf_selection):
    assert K.determinism(target) == 7


def test_arguments(target):
    assert K.arguments(target) == 14
