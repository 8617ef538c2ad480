"""The PNG writer on the MI355X: the checks of tests/png_write_checks.py over their whole matrices through the library's C ABI on
torch buffers, then the Engine layer (png_encode, save_png, png_bound)."""
import os

import pytest
import torch

import png_write_checks as K
from test_gpu_zip import TorchMem

pytestmark = pytest.mark.gpu


class GpuTarget(K.Target):
    def __init__(self):
        from zlib_rs_amd.engine import Engine
        self.e = Engine(0)
        super().__init__(self.e.L, self.e._ctx, TorchMem(self.e.device))


@pytest.fixture(scope="module")
def target():
    t = GpuTarget()
    yield t
    t.e.close()


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def test_geometry(target):
    """heights 1, 2, 63, 64, 65, 129 x widths 1, 2, 63, 64, 65; row_bytes around the trip in pixels of 1, 3, 4 and 8 bytes; row_bytes 1"""
    assert K.geometry(target) == 30 + 20 + 5


def test_formats(target):
    assert K.formats(target) == 2 * 14


def test_filters(target):
    assert K.filters(target) == 25


@pytest.mark.parametrize("native16", [True, False])
def test_long_rows(target, native16):
    assert K.long_rows(target, flags=(native16,)) == 66


@pytest.mark.parametrize("count", [1, 3, 64, 65, 300])
def test_batches(target, count):
    """every count at the input alignments 0, 1, 3, 15 with the output alignments 1, 16, 4096 in turn"""
    assert K.batches(target, counts=[count]) == 4


@pytest.mark.parametrize("level", [6, 9, 1, 0])
def test_pieces(target, level):
    assert K.pieces(target, levels=(level,)) == 9


def test_image_across_launch_groups(target):
    assert K.across_groups(target) == 41


def test_arguments(target):
    assert K.arguments(target) == 26


def test_statuses(target):
    assert K.statuses(target) == 6


def test_capacity(target):
    assert K.capacity(target) == 15


def test_determinism(target):
    assert K.determinism(target, _setenv, levels=(6, 1, 3)) == 18


@pytest.mark.parametrize("native16", [True, False])
def test_round_trip(target, native16):
    assert K.round_trip(target, native16) == 7


def test_engine(target):
    assert K.engine_layer(target.e, torch) == 5
