"""CPU tests of the TIFF writer (zmi_tiff_write_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/tiff_write_checks.py -- the ones tests/test_gpu_tiff_write.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here, as tests/test_emu_tiff.py thins the reader's, to the subsets named at
each test."""
import os

import pytest

import tiff_write_checks as K
import zmi_ctypes
from test_emu_zip import HostMem


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def _force_groups(count):
    def group_of(on):
        if on:
            os.environ["ZMI_STREAM_GROUP"] = str(count)
        else:
            os.environ.pop("ZMI_STREAM_GROUP", None)
    return group_of


def test_geometry(target):
    """tiles of 16 x 16 only (the GPU test adds 16 x 32); the strip cases; the row bytes around the predict tile for pixels of 3 and 6
    bytes, one 64-bit sample and float32 under predictor 3 (the GPU test adds pixels of 1, 4 and 8 bytes)"""
    assert K.geometry(target, tiles=((16, 16),), pixels=(K.PIXELS[1], K.PIXELS[3], K.PIXELS[5], K.PIXELS[6])) == 5 + 5 + 4 * 4


def test_formats(target):
    """every depth with 1 and 3 samples (the GPU test: 1 .. 4), the pages of 5, 7 and 8 samples, the PIL five"""
    assert K.formats(target, sample_counts=(1, 3)) == 4 + 3 * 6 + 7 + 5


def test_dense_and_assemble(target):
    """the input at shifts 0 and 3 (the GPU test: 0, 1, 3, 15)"""
    assert K.dense_and_assemble(target, shifts=(0, 3)) == 4


def test_pieces(target):
    """levels 6 and 0 (the GPU test: 1, 6, 9, 0)"""
    assert K.pieces(target, levels=(6, 0)) == 12


def test_launch_groups(target):
    """nine segments in pieces of 256 bytes are 27 pieces: forced launch groups of 10, which three of the segments lie across (the GPU
    test: a page of 30 MiB under the smallest scratch limit)"""
    c = K.Case(40, 40, 3, pred=2, tile=(16, 16), seed=13)
    assert K.across_groups(target, c, 256, 6, 10, _force_groups(10)) == 1


def test_determinism(target, inf_selection):
    assert K.determinism(target) == 4


def test_align(target):
    """alignments 1 and 4096 (the GPU test: 1, 2, 16, 4096)"""
    assert K.aligns(target, values=(1, 4096)) == 4


def test_inline_arrays(target):
    assert K.inline_arrays(target) == 4


def test_arguments(target):
    assert K.arguments(target) == 30 + 8


def test_capacity(target):
    assert K.capacity(target) == 8
