"""bench.py --dump-outputs: dump_outputs() and headline() on the CPU build of the kernels (tests/emu; device pointers = host pointers).
The dump must be float32 / float64 arrays that hold what the timed step handed its caller: every shard's compressed length,
status and CRC-32 of its stream, and the streams of a seeded sample of shards, zero past their ends."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, os, sys
ROOT = %(root)r
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import zlib_rs_amd._lib as zl
zl.LIB = os.path.join(ROOT, "tests", "emu", "libzmi355_emu.so")      # the same C ABI, compiled for the CPU (test infrastructure)
import zlib_rs_amd.engine as eng_mod
eng_mod._stream_ptr = lambda: None
import bench


class EmuEngine(eng_mod.Engine):
    def __init__(self):
        import ctypes as C
        self.device = torch.device("cpu")
        self.L = zl.lib()
        self._ctx = C.c_void_p()
        zl.check(self.L.zmi_ctx_create(C.byref(self._ctx), 0), "zmi_ctx_create")


class _Cuda:
    @staticmethod
    def synchronize(): pass


class TorchShim:
    cuda = _Cuda()
    def __getattr__(self, name): return getattr(torch, name)


e = EmuEngine()
S, B = 12, 8192
data = e.gen_shards(S, B)
off, ln = eng_mod.uniform_layout(S, B, torch.device("cpu"))
stride = e.deflate_bound(B, eng_mod.WRAP_ZLIB)
out = torch.full((S, stride), 0xA5, dtype=torch.uint8)               # (bytes past a stream's end must not reach the dump)
olen = torch.empty(S, dtype=torch.int32)
st = torch.empty(S, dtype=torch.int32)
e.deflate_batch(data, off, ln, B, level=6, wrap=eng_mod.WRAP_ZLIB, out=out, out_len=olen, status=st)
bench.dump_outputs(%(dir)r, e, TorchShim(), out, olen, st, budget=4 * stride * 5)   # room for 5 of the 8 sampled rows
open(os.path.join(%(dir)r, "streams.bin"), "wb").write(bytes(out.numpy()))


class Args:
    level, steps, warmup = 6, 4, 1


print(json.dumps(bench.headline(Args, 1, 2.0, S, B, 2.5, "checked")))
e.close()
'''


def test_dump_outputs_and_headline_on_the_emulator(tmp_path):
    import numpy as np
    import zlib
    import oracle_lib
    import zmi_ctypes
    zmi_ctypes.load_emu()                                            # (builds tests/emu/libzmi355_emu.so if needed)
    d = str(tmp_path / "dump")
    env = dict(os.environ, ZMI_TUNING="1")
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT, "dir": d}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == 4 and line["ms_per_step"] == 500.0 and line["value"] == 12 * 8192 * 4 / float(1 << 30) / 2.0

    S, B = 12, 8192
    names = sorted(f for f in os.listdir(d) if f.endswith(".npy"))
    assert names == ["compressed_crc32.npy", "out_len.npy", "sample_compressed.npy", "sample_shards.npy", "status.npy"]
    arrays = {n[:-4]: np.load(os.path.join(d, n)) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) < 64 << 20
    streams = open(os.path.join(d, "streams.bin"), "rb").read()
    stride = len(streams) // S
    lens = arrays["out_len"].astype(np.int64)
    assert lens.shape == (S,) and (arrays["status"] == 0).all()
    o = oracle_lib.load()
    for i in range(S):
        comp = streams[i * stride:i * stride + lens[i]]
        assert zlib.crc32(comp) == arrays["compressed_crc32"][i]
        assert zlib.decompress(comp) == o.gen_shard(i, B)
    idx = arrays["sample_shards"].astype(np.int64)
    rows = arrays["sample_compressed"]
    assert rows.shape == (5, stride) and len(set(idx.tolist())) == 5 and list(idx) == sorted(idx)
    for row, i in zip(rows, idx):
        assert bytes(row[:lens[i]].astype(np.uint8)) == streams[i * stride:i * stride + lens[i]]
        assert not row[lens[i]:].any()
