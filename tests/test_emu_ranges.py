"""CPU tests of zmi_inflate_stream_index_dev / zmi_inflate_ranges_dev on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/ranges_checks.py -- the ones tests/test_gpu_ranges.py runs on the MI355X.  The emulator runs a workgroup's threads as fibers, so
the matrices are thinned here: the range checks run over every fixture and both spans with the offset table, the stride and the odd
address on one of them; the jump resolve of a launch of a few ranges sweeps every byte its bitmap covers, so the launch groups of two
claimed 24 MiB regions run with it switched off (ZMI_INF_JUMP=0) -- the GPU runs them as the product does."""
import os

import numpy as np
import pytest

import ranges_checks as K
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


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def test_walker_counts_the_output(target):
    """the judge of the index: the walker's block starts are the scan's proposals, its output count is the payload's length"""
    f = K.fixture(target, "F1-raw")
    assert len(f.cuts) == 1 + 105 and f.offs == sorted(f.offs) and f.offs[-1] < 150000


@pytest.mark.parametrize("name", ["F1-gzip", "F2", "F4", "F5"])
def test_index_is_exact(target, inf_selection, name):
    full = name in ("F1-gzip", "F2") and inf_selection == "product"
    assert K.index_exact(target, name, setenv=_setenv if full else None, variants=inf_selection == "product") == (
        4 + 3 + 3 if full else (4 + 3 if inf_selection == "product" else 4))


def test_void_index(target, inf_selection):
    assert K.void_index(target) == 3


@pytest.mark.parametrize("span", [1, 40000])
@pytest.mark.parametrize("name", ["F1-raw", "F1-zlib", "F1-gzip", "F2"])
def test_ranges_are_exact(target, inf_selection, name, span):
    layouts = ((True, False), (False, False), (True, True)) if (name, span) == ("F1-gzip", 40000) else (((True, False),) if span == 1 else ((False, True),))
    assert K.ranges_exact(target, name, span, layouts=layouts) == 59 * len(layouts)


def test_independence(target, inf_selection, monkeypatch):
    assert K.independence(target, two_regions=False) == 3
    monkeypatch.setenv("ZMI_INF_JUMP", "0")
    assert K.independence(target, one_by_one=False) == 3


def test_windows_matter_and_may_be_withheld(target, inf_selection):
    assert K.windows(target) == 7


def test_truncation(target, inf_selection):
    assert K.truncation(target) == 4


@pytest.mark.parametrize("jump", ["0", "1"])
def test_a_few_ranges_under_either_resolve(target, monkeypatch, jump):
    """a launch of up to 16 ranges may take the pointer-jumping resolve: the same results from it and from the serial pass"""
    monkeypatch.setenv("ZMI_INF_JUMP", jump)
    assert K.windows(target) == 7 and K.truncation(target) == 4


def test_arguments(target):
    assert K.arguments(target) == 12 + 6 + 7
