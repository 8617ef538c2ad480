#!/usr/bin/env python3
"""Writing BGZF on the device, in one process on one MI355X: the generator's mix cut into --blocks x 65 280
bytes, level 6.
  bgzf        zmi_bgzf_deflate_dev (Engine.bgzf_compress into a preallocated buffer, with the index),
  yardstick   what a caller had before it: zmi_deflate_batch_dev(wrap gzip) on the same shards + zmi_pack_slab_dev -- a multi-member
              file with plain headers, no BSIZE, no index, no 64 KiB guarantee,
  stream      for scale, zmi_deflate_stream_dev in independent mode at 1 MiB pieces over the same bytes.
Warm-up first (the bgzf file is checked there: BSIZE chain, end-of-file block, and the whole file through the library's member
reader), HIP events, medians of --reps, the three alternating; then one more call of each of the first two with event timing on for
the per-slot kernel times (zmi_ctx_get_timing: 0 = CRC-32, 1 = match search, 5 = parse, 2 = encode, 7 = sizes / scan / pack / close).
Prints one JSON line and writes it to --out (default profiles/bgzf_deflate.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS = {0: "crc32", 1: "lz77", 5: "parse", 2: "encode", 7: "pack"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--block-bytes", type=int, default=65280)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_deflate.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlib_rs_amd import _lib
    from zlib_rs_amd.engine import Engine, uniform_layout, WRAP_GZIP
    e = Engine(0)
    L = _lib.lib()
    L.zmi_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.zmi_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    nb, bb = a.blocks, a.block_bytes
    raw = nb * bb
    # the generator writes shards of a multiple of 64 bytes: 1 MiB shards, the first `raw` bytes of them
    data = e.gen_shards(-(-raw // (1 << 20)), 1 << 20)[:raw]
    off, ln = uniform_layout(nb, bb, e.device)

    def timed(f):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), r

    def slots_of(f):
        sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)   # (drops what was recorded before)
        L.zmi_ctx_set_timing(e._ctx, 1)
        f()
        torch.cuda.synchronize()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)
        L.zmi_ctx_set_timing(e._ctx, 0)
        return {SLOTS[i]: round(sums[i], 3) for i in SLOTS}

    out = torch.empty(e.bgzf_bound(raw, bb), dtype=torch.uint8, device=e.device)
    stride = e.deflate_bound(bb, WRAP_GZIP)
    slots = torch.empty((nb, stride), dtype=torch.uint8, device=e.device)
    olen = torch.empty(nb, dtype=torch.int32, device=e.device)
    st = torch.empty(nb, dtype=torch.int32, device=e.device)
    slab = torch.empty(nb * stride // 2 + 16, dtype=torch.uint8, device=e.device)
    soff = torch.empty(nb + 1, dtype=torch.int64, device=e.device)
    sout = torch.empty(e.stream_bound(raw, 1 << 20, WRAP_GZIP), dtype=torch.uint8, device=e.device)

    def bgzf():
        return e.bgzf_compress(data, level=a.level, block_bytes=bb, index=True, out=out)

    def yard():
        e.deflate_batch(data, off, ln, bb, level=a.level, wrap=WRAP_GZIP, out=slots, out_len=olen, status=st)
        e.pack_slab(slots, olen, slab=slab, offsets=e.scan_sizes(olen, out=soff))
        return int(soff[nb].item())               # (the one synchronisation bgzf_compress has too)

    def stream():
        return e.deflate_stream(data, level=a.level, wrap=WRAP_GZIP, piece_bytes=1 << 20, independent=True, out=sout)

    ms = {"bgzf": [], "yardstick": [], "stream": []}
    sizes = {}
    for rep in range(a.reps + 1):                    # the first round is the warm-up and the check
        for k, f in (("bgzf", bgzf), ("yardstick", yard), ("stream", stream)):
            t, r = timed(f)
            if rep:
                ms[k].append(t)
                continue
            if k == "bgzf":
                file, index = r
                sizes[k] = int(file.numel())
                offs = np.array(index.block_off.tolist(), dtype=np.int64)
                host = file.cpu().numpy()
                bsize = host[offs[:-1] + 16].astype(np.int64) + (host[offs[:-1] + 17].astype(np.int64) << 8) + 1
                assert (offs[:-1] + bsize == offs[1:]).all() and offs[-1] + 28 == host.size and int(bsize.max()) <= bb + 31
                stored_blocks = int((host[offs[:-1] + 18] == 1).sum())
                back = e.inflate_members(file, starts=index.block_off)
                assert torch.equal(back, data)
                del back, host
            elif k == "yardstick":
                assert int((st != 0).sum().item()) == 0 and r <= slab.numel()
                sizes[k] = r
            else:
                sizes[k] = int(r.numel())
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"probe": "bgzf_deflate", "blocks": nb, "block_bytes": bb, "level": a.level, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "raw_bytes": raw, "stored_blocks": stored_blocks}
    for k in ms:
        res[k] = {"ms_median": round(med[k], 3), "ms_spread": round(max(ms[k]) - min(ms[k]), 3), "gib_s": round(raw / 2**30 / (med[k] / 1e3), 2),
                  "bytes": sizes[k], "ratio": round(raw / sizes[k], 4)}
    res["bgzf"]["slots_ms"] = slots_of(bgzf)
    res["yardstick"]["slots_ms"] = slots_of(yard)
    res["bgzf_over_yardstick"] = round(med["bgzf"] / med["yardstick"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
