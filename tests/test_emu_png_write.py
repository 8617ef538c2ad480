"""CPU tests of the PNG writer (zmi_png_encode_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/png_write_checks.py -- the ones tests/test_gpu_png_write.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test."""
import os

import pytest

import png_write_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


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


def test_geometry(target):
    """heights 1, 2, 64, 65 against widths 1, 63, 65 (the GPU test adds heights 63 and 129 and widths 2 and 64), and every trip case"""
    assert K.geometry(target, heights=(1, 2, 64, 65), widths=(1, 63, 65)) == 12 + 20 + 5


def test_formats(target):
    assert K.formats(target) == 2 * 14


def test_filters(target):
    assert K.filters(target) == 25


def test_long_rows(target):
    """little-endian 16-bit samples with every type and the choice; big-endian with Average, Paeth and the choice (the GPU test: all)"""
    assert K.long_rows(target, flags=(True,)) == 66
    assert K.long_rows(target, flags=(False,), filts=(3, 4, K.ADAPTIVE)) == 33


@pytest.mark.parametrize("count", [1, 3, 64, 65, 300])
def test_batches(target, count):
    """1, 3 and 65 images at the four input alignments with the output alignments 1, 16 and 4096 in turn; 64 at two, 300 at one"""
    shifts = K.SHIFTS if count in (1, 3, 65) else ([3, 15] if count == 64 else [15])
    assert K.batches(target, counts=[count], shifts=shifts) == len(shifts)


def test_pieces(target):
    """levels 6 and 0 (the GPU test: 6, 9, 1, 0)"""
    assert K.pieces(target, levels=(6, 0)) == 18


def test_large_image_beside_tiny_ones(target):
    """200 KB in pieces of 64 KiB between tiny images, in forced launch groups of 3 pieces, which its four pieces lie across (the GPU
    test: 3 MiB under the smallest scratch limit)"""
    assert K.across_groups(target, big=200 << 10, pb=65536, front=5, behind=6, setenv=_setenv, force=3) == 12


def test_arguments(target):
    assert K.arguments(target) == 26


def test_statuses(target):
    assert K.statuses(target) == 6


def test_capacity(target):
    assert K.capacity(target) == 15


def test_determinism(target):
    """level 6 (the GPU test adds level 1)"""
    assert K.determinism(target, _setenv, levels=(6,)) == 6


def test_round_trip(target):
    assert K.round_trip(target) == 7
