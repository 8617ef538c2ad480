#!/usr/bin/env python3
"""Batch deflate / inflate against one shared preset dictionary on the MI355X: ratio and throughput by record size.

Level 6; dictionary = the first 32 KiB of lcet10.txt; records cut from the rest of it, tiled to about 1 GiB.  For the record sizes
4 KiB, 64 KiB and 1 MiB: ratio and GiB/s (of raw input) of Engine.deflate_batch with and without the dictionary, and GiB/s of
Engine.inflate_batch with it.  Prints one JSON line (profiles/shared_dict.json keeps one).

The numbers are reported, not gated.  With 4 KiB records every workgroup of the match search hashes 27 KiB of dictionary in front
of 4 KiB of payload, so the 4 KiB deflate figure is far below the benchmark's headline by construction; a prebuilt hash state of
the dictionary is not part of this engine yet.

Every record size is measured by a child process of its own under a time limit; the first one that fails ends the run.
"""
import argparse
import json
import lzma
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [4096, 65536, 1 << 20]


def one(size, total, level, reps):
    import numpy as np
    import torch
    from zlib_rs_amd.engine import Engine, WRAP_RAW

    with lzma.open(os.path.join(ROOT, "tests", "golden", "fixtures", "lcet10.txt.xz")) as f:
        text = f.read()
    zdict, rest = text[:32768], text[32768:]
    rest = rest[:len(rest) // size * size] if len(rest) >= size else rest * (size // len(rest) + 1)
    n = max(1, total // size)
    e = Engine(0)
    dev = e.device
    src = torch.from_numpy(np.frombuffer(rest, dtype=np.uint8).copy()).to(dev)
    data = src.repeat(n * size // src.numel() + 1)[:n * size].contiguous()
    off = torch.arange(n, dtype=torch.int64, device=dev) * size
    ln = torch.full((n,), size, dtype=torch.int32, device=dev)
    d_dict = torch.from_numpy(np.frombuffer(zdict, dtype=np.uint8).copy()).to(dev)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        return best

    res = {"record_bytes": size, "records": n}
    keep = {}
    for name, zd in (("deflate_dict", d_dict), ("deflate_plain", None)):
        stride = e.deflate_bound(size, WRAP_RAW, zdict=zd is not None)
        out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        olen = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        dt = timed(lambda: e.deflate_batch(data, off, ln, size, level=level, wrap=WRAP_RAW, out=out, out_len=olen, status=st, zdict=zd))
        assert int(st.abs().max().item()) == 0, name
        res[name + "_gibs"] = round(n * size / dt / 2 ** 30, 2)
        res[name + "_ratio"] = round(n * size / float(olen.sum(dtype=torch.int64).item()), 4)
        if zd is not None:
            keep = {"out": out, "olen": olen, "stride": stride}
        else:
            del out
    back = torch.empty(n * size, dtype=torch.uint8, device=dev)
    coff = torch.arange(n, dtype=torch.int64, device=dev) * keep["stride"]
    cap = torch.full((n,), size, dtype=torch.int32, device=dev)
    blen = torch.empty(n, dtype=torch.int32, device=dev)
    bst = torch.empty(n, dtype=torch.int32, device=dev)
    dt = timed(lambda: e.inflate_batch(keep["out"], coff, keep["olen"], back, off, cap, wrap=WRAP_RAW, out_len=blen, status=bst, zdict=d_dict))
    assert int(bst.abs().max().item()) == 0 and torch.equal(back, data), "inflate"
    res["inflate_dict_gibs"] = round(n * size / dt / 2 ** 30, 2)
    e.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=1 << 30, help="bytes of records per size")
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds one record size may take")
    ap.add_argument("--one", type=int, default=0, help="(child) measure this record size")
    a = ap.parse_args()
    if a.one:
        one(a.one, a.total, a.level, a.reps)
        return 0
    rows = []
    for size in SIZES:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(size), "--total", str(a.total), "--level", str(a.level),
                                "--reps", str(a.reps)], stdout=subprocess.PIPE, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps({"error": "time limit", "record_bytes": size, "sizes": rows}))
            return 124
        if p.returncode != 0:
            print(json.dumps({"error": "exit %d" % p.returncode, "record_bytes": size, "sizes": rows}))
            return 1
        rows.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    print(json.dumps({"probe": "shared_dict", "level": a.level, "dict_bytes": 32768, "text": "lcet10.txt", "sizes": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
