"""Probe of the batch inflate without an output size table (one JSON document; kept as profiles/inflate_sizes.json).

gen_shards (default 16 384 x 1 MiB) is deflated by the library itself with the zlib wrapper at level 6, level 1 (fixed blocks) and level 0
(stored), and every input is inflated three ways in one process:
  (a) inflate_batch with the true offset / size table;
  (b) inflate_sizes -- the size pass alone;
  (c) inflate_batch_packed into a buffer of exactly the right size (size pass + plan + decode).
Each leg is warmed up, then five rounds alternate a, b, c; a leg is timed with device events around the call, ending in a synchronise.
Reported per leg: the median and the spread (max - min) of the rounds, and the per-kernel sums of zmi_ctx_get_timing (slot 3 = the decode
kernel, which is also where the size pass is counted).  The sizes of (b) must equal the true lengths and the bytes of (a) and (c) the data.
There is no speed gate: the figure of interest is (b) against slot 3 of (a) in the same run.

    python tools/gpu_inflate_sizes_probe.py [--shards N] [--shard-bytes B] [--rounds R] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["checksum", "lz77", "encode", "decode", "verify", "plan", "resolve", "offset_scan"]


def median(v):
    return sorted(v)[len(v) // 2]


def measure(e, level, args):
    import torch
    from zlib_rs_amd.engine import uniform_layout, WRAP_ZLIB
    n, shard = args.shards, args.shard_bytes
    data = e.gen_shards(n, shard)
    off, ln = uniform_layout(n, shard, e.device)
    slots, clen, st = e.deflate_batch(data, off, ln, shard, level=level, wrap=WRAP_ZLIB)
    assert int((st != 0).sum().item()) == 0
    coff = torch.arange(n, dtype=torch.int64, device=e.device) * slots.stride(0)
    back = torch.empty(n * shard, dtype=torch.uint8, device=e.device)
    cap = torch.full((n,), shard, dtype=torch.int32, device=e.device)
    ooff = torch.arange(n, dtype=torch.int64, device=e.device) * shard
    keep = {}

    def leg_a():
        keep["a"] = e.inflate_batch(slots, coff, clen, back, ooff, cap, wrap=WRAP_ZLIB)

    def leg_b():
        keep["b"] = e.inflate_sizes(slots, coff, clen, wrap=WRAP_ZLIB)

    def leg_c():
        keep["c"] = e.inflate_batch_packed(slots, coff, clen, wrap=WRAP_ZLIB, out=back)

    legs = (("a", leg_a), ("b", leg_b), ("c", leg_c))
    sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        e.L.zmi_ctx_get_timing(e._ctx, sums, counts)
        return a.elapsed_time(b), {NAMES[k]: sums[k] for k in range(8) if counts[k]}

    # warm-up, with the correctness checks
    for name, fn in legs:
        back.zero_()
        once(fn)
        if name == "a":
            assert int((keep["a"][1] != 0).sum().item()) == 0 and torch.equal(back, data)
        elif name == "b":
            sizes, sst = keep["b"]
            assert int((sst != 0).sum().item()) == 0 and torch.equal(sizes, ln)
        else:
            out, poff, plen, pst = keep["c"]
            assert int((pst != 0).sum().item()) == 0 and torch.equal(plen, ln) and torch.equal(poff[:n], ooff) and int(poff[n].item()) == n * shard
            assert torch.equal(back, data)
    ms = {name: [] for name, _ in legs}
    slot = {name: [] for name, _ in legs}
    for _ in range(args.rounds):
        for name, fn in legs:
            t, k = once(fn)
            ms[name].append(t)
            slot[name].append(k)
    res = {"level": level, "compressed_bytes": int(clen.to(torch.int64).sum().item())}
    for name, _ in legs:
        res[name] = {"median_ms": round(median(ms[name]), 3), "spread_ms": round(max(ms[name]) - min(ms[name]), 3),
                     "rounds_ms": [round(t, 3) for t in ms[name]],
                     "kernel_median_ms": {k: round(median([s.get(k, 0.0) for s in slot[name]]), 3) for k in slot[name][0]}}
    a3 = [s["decode"] for s in slot["a"]]
    res["a_decode_kernel_median_ms"] = round(median(a3), 3)
    res["a_decode_kernel_spread_ms"] = round(max(a3) - min(a3), 3)
    res["b_over_a_decode_kernel"] = round(median(ms["b"]) / median(a3), 4)
    res["c_over_a"] = round(median(ms["c"]) / median(ms["a"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=16384)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--levels", default="6,1,0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_sizes.json"))
    args = ap.parse_args()
    from zlib_rs_amd.engine import Engine
    e = Engine(0)
    e.L.zmi_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    e.L.zmi_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    e.L.zmi_ctx_set_timing(e._ctx, 1)
    res = {"shards": args.shards, "shard_bytes": args.shard_bytes, "rounds": args.rounds, "wrap": "zlib",
           "inputs": [measure(e, int(level), args) for level in args.levels.split(",")]}
    e.close()
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
