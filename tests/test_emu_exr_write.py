"""CPU tests of the OpenEXR writer (zmi_exr_bound / zmi_exr_write_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/exr_write_checks.py -- the ones tests/test_gpu_exr_write.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import os

import pytest

import exr_write_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def _set_group(pieces):
    if pieces:
        os.environ["ZMI_STREAM_GROUP"] = str(pieces)
    else:
        os.environ.pop("ZMI_STREAM_GROUP", None)


def test_geometry(target):
    """widths 1, 3, 65 and 257, heights 1, 17 and 33, every compression and channel layout (the GPU test adds widths 2, 5, 17, 63 and 64
    and heights 15 and 16)"""
    assert K.geometry(target, widths=(1, 3, 65, 257), heights=(1, 17, 33)) == 3 * 3 * 4 * 3


def test_trips(target):
    """ZIP only (the GPU test adds ZIPS), and the four seams"""
    assert K.trips(target, comps=(K.ZIP,)) == 6 + 4


def test_tiles(target):
    assert K.tiles(target) == 8


def test_raw_rule(target):
    assert K.raw_rule(target) == 5


def test_pieces(target):
    """levels 6 and 0 (the GPU test: 1, 6, 9, 0)"""
    assert K.pieces(target, levels=(6, 0)) == 4


def test_launch_groups(target):
    assert K.launch_groups(target, _set_group) == 3


def test_independence(target):
    """shifts 0 and 3 (the GPU test: 0, 1, 3, 15)"""
    assert K.independence(target, shifts=(0, 3)) == 2 + 3


def test_pin(target):
    assert K.pin(target) == 1


def test_capacity(target):
    """alignments 1 and 4096 (the GPU test adds 16)"""
    assert K.capacity(target, aligns=(1, 4096)) == 8


def test_arguments(target):
    assert K.arguments(target) == 32 + 8 + 3
