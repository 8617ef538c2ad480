"""CPU tests of the decode kernels on hand-built dynamic-Huffman blocks (tests/deflate_craft.py, tests/dynamic_block_checks.py) on the
emulator build: 48-bit tokens, tables of exactly 852 and 400 entries, the single-code forms, every header shape, 300 tiny blocks
and deliberately placed errors through the batch decode, the size pass, the packed decode, the resumable decode, the block scan
and the single-stream decode.  tests/test_gpu_dynamic_blocks.py runs the same checks on the MI355X; the judge is the oracle and
deflate_craft.inflate_ref (tests/test_deflate_craft.py), never the library."""
import pytest

import dynamic_block_checks as K
import oracle_lib
import zmi_ctypes
from test_emu_inflate_sizes import EmuTarget
from test_emu_stream_inflate_blocks import _Ctx, _bind


@pytest.fixture(scope="module")
def eng():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield e
    e.close()


@pytest.fixture(scope="module")
def target():
    t = EmuTarget()
    yield t
    t.close()


@pytest.fixture(scope="module")
def ctx(eng):
    c = _Ctx(_bind(eng.lib))
    yield c
    c.close()


@pytest.fixture(scope="module")
def o():
    return oracle_lib.load()


def test_batch_decode_is_exact(eng, o, inf_selection):
    assert K.batch_exact(eng.inflate, o) > 100


def test_words_of_the_size_pass_and_the_packed_decode_are_exact(target, o, inf_selection):
    assert K.words_exact(target, o, shifts=(None,)) > 100


def test_resume_is_exact(eng, inf_selection):
    assert K.resume_exact(eng) >= 10


def test_block_scan_and_block_decode_are_exact(ctx, eng, inf_selection):
    assert K.scan_exact(ctx, eng) == 3
