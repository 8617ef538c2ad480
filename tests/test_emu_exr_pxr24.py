"""CPU tests of OpenEXR PXR24 (compression 5) in the reader and the writer on the emulator build (tests/emu/, -DZMI_EMU) with the checks
of tests/exr_pxr24_checks.py -- the ones tests/test_gpu_exr_pxr24.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test; the other checks run whole."""
import os

import pytest

import exr_pxr24_checks as K
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


def test_read_geometry(target):
    """widths 1, 3, 65, T - 1, T + 1 and 2 T + 1, heights 1, 16 and 17 (the GPU test adds widths 2, 5, 63, 64 and T, heights 15 and 33)"""
    T = target.p24_trip
    assert K.read_geometry(target, widths=(1, 3, 65, T - 1, T + 1, 2 * T + 1), heights=(1, 16, 17)) == 5 * 6 * 3


def test_read_tiles(target):
    assert K.read_tiles(target) == 10


def test_read_values(target):
    assert K.read_values(target) == 12


def test_read_raw_chunks(target):
    assert K.read_raw_chunks(target) == 4


def test_read_faults(target):
    assert K.read_faults(target) == 7


def test_read_independence(target, inf_selection):
    assert K.read_independence(target) == 4 + 2 + 6


def test_write_geometry(target):
    """widths 3, 65 and 2 T + 1, heights 1 and 17, three layouts (the GPU test: eleven widths, five heights, five layouts)"""
    T = target.p24_trip
    assert K.write_geometry(target, widths=(3, 65, 2 * T + 1), heights=(1, 17), layouts=(K.RGBA, K.MIXED, K.ONE_FLOAT)) == 3 * 3 * 2


def test_write_tiles(target):
    assert K.write_tiles(target) == 4


def test_write_values(target):
    assert K.write_values(target) == 11


def test_write_raw_rule(target):
    assert K.write_raw_rule(target) == 4


def test_write_pieces_and_launch_groups(target):
    """level 6 (the GPU test: 1, 6, 9, 0)"""
    assert K.write_pieces(target, levels=(6,), set_group=_set_group) == 4 + 2


def test_write_independence(target):
    """shifts 0 and 3 (the GPU test: 0 .. 3)"""
    assert K.write_independence(target, shifts=(0, 3)) == 3
