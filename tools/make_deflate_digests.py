"""Writes tests/golden/deflate_digests.json: length and SHA-256 of what the CPU emulator build compresses the inputs of
tests/schedule_checks.py to, per (input, level) -- the bytes tests/test_emu_schedule.py and tests/test_gpu_schedule.py hold the emulator
and the MI355X to.  A change that alters compressed bytes on purpose runs this and commits the file with the change.
usage: python tools/make_deflate_digests.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("ZMI_TUNING", "1")
os.environ.pop("ZMI_EMU_SCHED", None)
os.environ.pop("ZMI_PRODUCERS", None)
import schedule_checks as K  # noqa: E402
import zmi_ctypes  # noqa: E402
from test_emu_bgzf import HostMem  # noqa: E402

K.oracle_lib.load()
eng = zmi_ctypes.Engine(zmi_ctypes.load_emu())
doc = {"wrap": K.WRAP_ZLIB, "levels": K.LEVELS, "inputs": [[name, len(b)] for name, b in K.inputs()],
       "digests": K.digests_of(K.Target(eng.lib, eng.ctx, HostMem()))}
with open(K.DIGESTS, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", K.DIGESTS)
