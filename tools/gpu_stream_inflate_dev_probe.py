#!/usr/bin/env python3
"""Single-stream inflate on the device against the batch API, in one process: 16 384 x 1 MiB generated shards at level 6, gzip, as
  batch     zmi_inflate_batch_dev over the shards as independent gzip members (zmi_deflate_batch_dev's output),
  carry     Engine.inflate_stream (zmi_inflate_stream_dev) of Engine.deflate_stream's carry-over stream, with its piece index,
  indep     the same for the ZMI_STREAM_INDEPENDENT stream,
alternating, timed with HIP events, median of --reps; every result is compared with the input once.  Per-stage kernel times of one
more call of each stream form come from the context's timers (zmi_ctx_get_timing: decode = kernel 3, symbolic resolve = 6, window
scan = 5, substitute + offsets = 7, checksums = 0, header / setup / verification / trailer = 4).  Prints one JSON line (GiB/s of
output per form) and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = {0: "checksum", 3: "decode", 4: "verify", 5: "window_scan", 6: "symbolic_resolve", 7: "substitute_offsets"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=16384)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from zlib_rs_amd import _lib
    from zlib_rs_amd.engine import Engine, uniform_layout, WRAP_GZIP
    e = Engine(0)
    L = _lib.lib()
    L.zmi_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.zmi_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    n, B = a.shards, a.shard_bytes
    raw = n * B
    data = e.gen_shards(n, B)
    off, ln = uniform_layout(n, B, e.device)
    slots, olen, st = e.deflate_batch(data, off, ln, B, level=a.level, wrap=WRAP_GZIP)
    torch.cuda.synchronize()
    assert int((st != 0).sum().item()) == 0
    coff = torch.arange(n, dtype=torch.int64, device=e.device) * slots.stride(0)
    ooff = torch.arange(n, dtype=torch.int64, device=e.device) * B
    ocap = torch.full((n,), B, dtype=torch.int32, device=e.device)
    streams = {}
    for k, indep in (("carry", False), ("independent", True)):
        s, idx = e.deflate_stream(data, level=a.level, wrap=WRAP_GZIP, piece_bytes=B, independent=indep, index=True)
        streams[k] = (s.clone(), idx[:-1].clone())
        del s, idx
    torch.cuda.synchronize()
    back = torch.empty(raw, dtype=torch.uint8, device=e.device)

    def batch():
        e.inflate_batch(slots, coff, olen, back, ooff, ocap, wrap=WRAP_GZIP)

    def stream(k):
        s, idx = streams[k]
        return lambda: e.inflate_stream(s, wrap=WRAP_GZIP, index=idx, piece_out_max=B, out=back)

    forms = {"batch_members": batch, "stream_carry": stream("carry"), "stream_independent": stream("independent")}
    ms = {k: [] for k in forms}
    for rep in range(a.reps + 1):                    # the first round is the warm-up and the check
        for k, f in forms.items():
            back.fill_(0)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                ms[k].append(t0.elapsed_time(t1))
            else:
                assert torch.equal(back, data), k
    res = {"probe": "stream_inflate_dev", "shards": n, "shard_bytes": B, "level": a.level, "wrap": "gzip", "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for k in forms:
        med = statistics.median(ms[k])
        res[k] = {"ms_median": round(med, 3), "gib_s": round(raw / 2**30 / (med / 1e3), 2)}
    for k in ("carry", "independent"):
        sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)   # (drops what was recorded before)
        L.zmi_ctx_set_timing(e._ctx, 1)
        forms["stream_" + k]()
        torch.cuda.synchronize()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)
        L.zmi_ctx_set_timing(e._ctx, 0)
        stages = {STAGES[i]: round(sums[i], 3) for i in STAGES}
        tot = sum(stages.values())
        res["stages_ms_" + k] = stages
        res["window_scan_share_" + k] = round(stages["window_scan"] / tot, 4) if tot else None
    res["carry_vs_batch"] = round(res["stream_carry"]["gib_s"] / res["batch_members"]["gib_s"], 3)
    res["independent_vs_batch"] = round(res["stream_independent"]["gib_s"] / res["batch_members"]["gib_s"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
