"""CPU tests of schedule independence on the emulator build (tests/emu/, -DZMI_EMU) with the checks of tests/schedule_checks.py.

The emulator runs one schedule -- every pass resumes the runnable fibers in thread order -- unless ZMI_EMU_SCHED perturbs it
(tests/emu/hip_emu.h: whole waves held back for given passes, or at random from a seed).  Deflate's match search (csrc/lz77.hip) is
producer and searcher waves talking through LDS flags and spin waits; what it writes must be the same bytes under every schedule and
with every number of producer waves, and those bytes are the committed ones (tests/golden/deflate_digests.json), which the MI355X must
give as well (tests/test_gpu_schedule.py).  The other kernels with spin waits or several waves per workgroup run once under the same
schedules, and the scheduler itself is checked on four kernels of its own (tests/emu/sched_selftest.cpp)."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import schedule_checks as K
import zmi_ctypes
from test_emu_bgzf import HostMem

EMU = os.path.join(zmi_ctypes.ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def engine():
    K.oracle_lib.load()                    # (builds the oracle where it is not built yet: inputs() takes two shards from its generator)
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield e
    e.close()


@pytest.fixture(scope="module")
def target(engine):
    return K.Target(engine.lib, engine.ctx, HostMem())


@pytest.mark.parametrize("level", K.LEVELS)
def test_deflate_bytes_do_not_depend_on_the_schedule(target, level):
    """inputs() under 11 schedules x 5 producer counts: every stream inflates to its input, and per input all 55 are the same bytes.
    (Before the emulator resumed a wave's lanes in one pass after every release -- hip_emu.h, resume_in_a_later_pass -- hold:0:1:1
    changed every text input at every level, e.g. lcet10[:65280] at level 6: 23 092 -> 23 168 bytes; with that and the parent commit's
    lz77.hip, hold:3:3:3000 at three producers and seed:6:800 / seed:3:500 at three / four changed lcet10[:40000] at level 1:
    16 122 -> 16 130 / 16 121 / 16 131 bytes.)"""
    assert K.schedule_invariance(target, level) == len(K.PRODUCERS) * len(K.SCHEDULES) == 55


def test_emulator_reproduces_the_committed_digests(target):
    """a change of compressed bytes shows here first: tools/make_deflate_digests.py regenerates the file"""
    assert K.check_digests(target) == 5 * 10


# ---- the other kernels with spin waits or several waves per workgroup ------------------------------------------------------------------------
def test_inflate_pack_and_scan_under_the_same_schedules(engine):
    """one small batch inflate (fixed, dynamic and stored blocks; 20 streams: the 16-wave kernel, and under ZMI_INF_MW_MAX=16 the
    one-wave kernel), one pack_slab and one scan_sizes call of more than one 1024-thread pass: the plain answers under every schedule.
    (A DEADLOCK or LIVELOCK report aborts the process.)"""
    raws = [K.text()[i * 700:i * 700 + 300 + 613 * i] for i in range(18)] + [bytes(3000), bytes(range(256)) * 9]
    streams = [zlib.compress(r, (1, 6, 9, 0)[i % 4]) for i, r in enumerate(raws)]
    members = [s[:len(s) - (i % 3)] for i, s in enumerate(streams)]
    lens = np.array([(i * 2654435761) % 70001 for i in range(2500)], dtype=np.uint32)
    want_scan = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    engine.lib.zmi_scan_sizes_dev.argtypes = [K.C.c_void_p, K.C.c_void_p, K.C.c_uint32, K.C.c_void_p, K.C.c_void_p]
    try:
        for sched in K.SCHEDULES:
            K.setenv("ZMI_EMU_SCHED", sched)
            for mw in (None, "16"):
                K.setenv("ZMI_INF_MW_MAX", mw)
                out, st = engine.inflate(streams, [len(r) for r in raws])
                assert st == [0] * len(raws) and out == raws, (sched, mw)
            slab, off = engine.pack_slab(members, 16384, slot_base=3, slab_base=5)
            assert slab == b"".join(members) and off == [sum(len(m) for m in members[:i]) for i in range(len(members) + 1)], sched
            got = np.full(len(lens) + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            assert engine.lib.zmi_scan_sizes_dev(engine.ctx, lens.ctypes.data, len(lens), got.ctypes.data, None) == 0
            assert np.array_equal(got, want_scan), sched
    finally:
        K.setenv("ZMI_EMU_SCHED", None)
        K.setenv("ZMI_INF_MW_MAX", None)


# ---- the scheduler itself --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "sched_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", EMU, "-o", exe, os.path.join(EMU, "sched_selftest.cpp"),
                    os.path.join(EMU, "hip_emu.cpp")], check=True)

    def run(mode, sched):
        env = dict(os.environ)
        env.pop("ZMI_EMU_SCHED", None)
        if sched:
            env["ZMI_EMU_SCHED"] = sched
        return subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=120)
    return run


SELF_SCHEDULES = [None, "hold:0:1:1", "hold:0:1:50", "hold:1:1:5", "hold:1:3:40", "seed:1", "seed:2", "seed:3:500", "seed:6:800"]


@pytest.mark.parametrize("sched", SELF_SCHEDULES)
def test_lanes_of_a_wave_stay_in_step(selftest, sched):
    """64 lanes store to one LDS cell after a barrier and after rendezvous: the highest lane's value stays, in both waves of both blocks
    (a wave held through the first pass used to come out of the barrier with lane 63 a pass ahead, and lane 62 won); a wave that spins
    on another wave's flag gets the value"""
    r = selftest("order", sched)
    assert r.returncode == 0 and r.stdout.split() == [str(63 + 100 * k) for k in (0, 1, 2)] * 4, (r.stdout, r.stderr)
    r = selftest("flag", sched)
    assert r.returncode == 0 and r.stdout.split() == ["2016", "2016"], (r.stdout, r.stderr)


@pytest.mark.parametrize("sched", [None, "hold:0:1:50", "hold:1:2:7", "seed:1", "seed:6:800"])
def test_a_real_deadlock_is_still_reported(selftest, sched):
    r = selftest("deadlock", sched)
    assert r.returncode == -6 and "[hip_emu] DEADLOCK in block 0: 128 threads parked" in r.stderr, (r.returncode, r.stderr)


def test_a_real_livelock_is_still_reported(selftest):
    r = selftest("livelock", "seed:3:500")
    assert r.returncode == -6 and "[hip_emu] LIVELOCK in block 0: 64 threads only spin-waiting" in r.stderr, (r.returncode, r.stderr)


def test_a_malformed_knob_is_refused(selftest):
    for bad in ("hold:0:1", "hold:0:0:1", "seed:", "seed:1:1001", "skip:3", "hold:0:1:1x"):
        r = selftest("order", bad)
        assert r.returncode == -6 and "ZMI_EMU_SCHED=" + bad in r.stderr, (bad, r.returncode, r.stderr)
