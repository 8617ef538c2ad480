"""Probe of the multi-member gzip inflate on the device (one JSON line; kept as profiles/members_inflate.json).

The stitched gzip output of deflate_batch over gen_shards (default 16 384 x 1 MiB, level 6) is inflated two ways:
  (a) inflate_batch with the true offset / size table -- the ceiling, the table being what a written file no longer has;
  (b) find_members + inflate_members from the bytes alone.
Per-stage times of (b) -- scan, plan, decode (with resolve and CRC-32), verify -- come from the context's event timing
(zmi_ctx_get_timing: kernel classes, include/zmi355.h); the cost of the idle repair passes is (b) with ZMI_MM_REPAIR_PASSES passes minus (b) with none (the tuning override ZMI_MM_REPAIR, read in
processes started with ZMI_TUNING), measured in child processes of this tool.

    python tools/gpu_members_probe.py [--shards N] [--shard-bytes B] [--reps R]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import torch
    from zlib_rs_amd.engine import Engine, uniform_layout, WRAP_GZIP
    e = Engine(0)
    n, shard = args.shards, args.shard_bytes
    data = e.gen_shards(n, shard)
    off, ln = uniform_layout(n, shard, e.device)
    slots, clen, st = e.deflate_batch(data, off, ln, shard, level=6, wrap=WRAP_GZIP)
    assert int((st != 0).sum().item()) == 0
    slab, coff = e.pack_slab(slots, clen)
    del slots
    total_c = int(coff[n].item())
    file = slab[:total_c]
    back = torch.empty(n * shard, dtype=torch.uint8, device=e.device)
    cap = torch.full((n,), shard, dtype=torch.int32, device=e.device)
    ooff = torch.arange(n, dtype=torch.int64, device=e.device) * shard

    def timed(fn):
        times = []
        for i in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i:
                times.append(a.elapsed_time(b))
        return sorted(times)[len(times) // 2]

    def leg_a():
        blen, bst = e.inflate_batch(file, coff[:n], clen, back, ooff, cap, wrap=WRAP_GZIP)
        return bst

    ms_a = timed(leg_a)
    assert torch.equal(back, data)
    back.zero_()
    found = {}

    def leg_scan():
        found["s"] = e.find_members(file, cap=n + 1024)

    def leg_inflate():
        found["r"] = e.inflate_members_raw(file, found["s"], back)

    ms_scan = timed(leg_scan)
    ms_inf = timed(leg_inflate)
    status, kind, idx, members, used, olen = found["r"]
    assert (status, members, used, olen) == (0, n, total_c, n * shard), found["r"]
    assert torch.equal(back, data)
    # stages of one inflate_members call, by kernel class
    sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()
    e.L.zmi_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    e.L.zmi_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    e.L.zmi_ctx_set_timing(e._ctx, 1)
    leg_inflate()
    e.L.zmi_ctx_get_timing(e._ctx, sums, counts)
    e.L.zmi_ctx_set_timing(e._ctx, 0)
    # (include/zmi355.h: 5 = plan and group setup; 4 = verify: the batch's trailer check, the chain verify and the repair kernels of all
    # passes; the repair PASSES as a whole are the difference to a run without them, below)
    names = ["crc32", "lz77", "encode", "decode", "verify", "plan", "resolve", "offset_scan"]
    stages = {names[k]: round(sums[k], 3) for k in range(8) if counts[k]}
    stages["scan"] = round(ms_scan, 3)
    res = {"shards": n, "shard_bytes": shard, "compressed_bytes": total_c, "proposals": int(found["s"].numel()),
           "false_proposals": int(found["s"].numel()) - n, "table_ms": round(ms_a, 3), "scan_ms": round(ms_scan, 3),
           "inflate_members_ms": round(ms_inf, 3), "members_ms": round(ms_scan + ms_inf, 3),
           "ratio_b_over_a": round((ms_scan + ms_inf) / ms_a, 4), "scan_gb_s": round(total_c / ms_scan / 1e6, 1),
           "stages_ms": stages, "repair_passes": os.environ.get("ZMI_MM_REPAIR", "default")}
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=16384)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    runs = {}
    for label, env in (("default", {}), ("no_repair", {"ZMI_TUNING": "1", "ZMI_MM_REPAIR": "0"})):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shards", str(args.shards), "--shard-bytes",
                            str(args.shard_bytes), "--reps", str(args.reps)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        runs[label] = json.loads(p.stdout.strip().splitlines()[-1])
    res = runs["default"]
    idle = res["inflate_members_ms"] - runs["no_repair"]["inflate_members_ms"]
    res["idle_repair_passes_ms"] = round(idle, 3)
    res["idle_repair_share_of_b"] = round(idle / res["members_ms"], 4)
    res["no_repair_inflate_members_ms"] = runs["no_repair"]["inflate_members_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
