"""Schedule independence of deflate on the MI355X, with the checks of tests/schedule_checks.py: the device has no schedule knob, so
what can be compared is one call with the next, one number of producer waves with another (csrc/lz77.hip; ZMI_PRODUCERS is read per
call under ZMI_TUNING), and the device with the CPU emulator, whose bytes per (input, level) are committed as
tests/golden/deflate_digests.json (tests/test_emu_schedule.py holds the emulator to the same file).  These tests repeat a correct
operation a few times to compare bytes; they are not a loop that waits for something to go wrong."""
import pytest

import schedule_checks as K
from test_gpu_bgzf import TorchMem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def target():
    from zlib_rs_amd.engine import Engine
    e = Engine(0)
    yield K.Target(e.L, e._ctx, TorchMem(e.device))
    e.close()


@pytest.mark.parametrize("level", K.LEVELS)
def test_five_calls_give_the_same_bytes(target, level):
    """the product's producer count (three at levels 1 and 3, where five calls used to give different streams:
    profiles/bgzf_level1_reproducibility.txt), four sets of shards"""
    assert sorted(K.repeat_calls(target, level)) == ["4 x 65280", "48 x 4096", "8 classes", "ragged"]


@pytest.mark.parametrize("level", K.LEVELS)
def test_bytes_do_not_depend_on_the_number_of_producers(target, level):
    assert K.producer_counts(target, level) == 4 * 4


def test_device_gives_the_emulators_bytes(target):
    assert K.check_digests(target) == 5 * 10
