#!/usr/bin/env python3
"""Single-stream deflate on the device against the batch API, in one process: 16 384 x 1 MiB generated shards at level 6 as
  batch     zmi_deflate_batch_dev, zlib wrapper (independent members -- bench.py's leg),
  carry     Engine.deflate_stream (zmi_deflate_stream_dev), zlib wrapper, carry-over pieces of 1 MiB,
  indep     the same with ZMI_STREAM_INDEPENDENT,
alternating, timed with HIP events, median of --reps.  Prints one JSON line (GiB/s of raw input and ratio per form) and writes it to
--out.  For the new kernels' share run it once more under `rocprofv3 --kernel-trace --stats -- python tools/gpu_stream_dev_probe.py
--reps 1` and read zmi_combine_kernel / zmi_frame_kernel in the stats."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=16384)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from zlib_rs_amd.engine import Engine, uniform_layout, WRAP_ZLIB
    e = Engine(0)
    n, B = a.shards, a.shard_bytes
    data = e.gen_shards(n, B)
    off, ln = uniform_layout(n, B, e.device)
    raw = n * B
    stride = e.deflate_bound(B, WRAP_ZLIB)
    slots = torch.empty((n, stride), dtype=torch.uint8, device=e.device)
    olen = torch.empty(n, dtype=torch.int32, device=e.device)
    st = torch.empty(n, dtype=torch.int32, device=e.device)
    sout = torch.empty(e.stream_bound(raw, B, WRAP_ZLIB), dtype=torch.uint8, device=e.device)
    torch.cuda.synchronize()

    def batch():
        e.deflate_batch(data, off, ln, B, level=a.level, wrap=WRAP_ZLIB, out=slots, out_len=olen, status=st)
        return None

    def carry():
        return int(e.deflate_stream(data, level=a.level, wrap=WRAP_ZLIB, piece_bytes=B, out=sout).numel())

    def indep():
        return int(e.deflate_stream(data, level=a.level, wrap=WRAP_ZLIB, piece_bytes=B, independent=True, out=sout).numel())

    forms = {"batch_zlib": batch, "stream_carry": carry, "stream_independent": indep}
    ms = {k: [] for k in forms}
    size = {}
    for rep in range(a.reps + 1):                    # the first round is the warm-up
        for k, f in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = f()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                ms[k].append(t0.elapsed_time(t1))
            if k == "batch_zlib":
                assert int((st != 0).sum().item()) == 0
                r = int(olen.to(torch.int64).sum().item())
            size[k] = r
    res = {"probe": "stream_deflate_dev", "shards": n, "shard_bytes": B, "level": a.level, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for k in forms:
        med = statistics.median(ms[k])
        res[k] = {"ms_median": round(med, 3), "gib_s": round(raw / 2**30 / (med / 1e3), 2), "ratio": round(raw / size[k], 4)}
    res["carry_vs_batch"] = round(res["stream_carry"]["gib_s"] / res["batch_zlib"]["gib_s"], 3)
    res["independent_vs_batch"] = round(res["stream_independent"]["gib_s"] / res["batch_zlib"]["gib_s"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
