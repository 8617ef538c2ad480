#!/usr/bin/env python3
"""Random access into one deflate stream on the device, in one process: a --shards x 1 MiB level-6 gzip carry
stream from Engine.deflate_stream (the data of tools/gpu_stream_inflate_dev_probe.py), decoded through its piece index as bit cuts.
  index cost   zmi_inflate_stream_index_dev at span 1 MiB against zmi_inflate_stream_bits_dev on the same arguments, alternating; the
               difference of the medians beside the run-to-run spread of the plain call,
  range reads  4096 seeded ranges of 64 KiB and 256 of 1 MiB through Engine.read_ranges into a preallocated buffer: ms, GiB/s of bytes
               delivered, GiB/s of bytes decoded (skip + len), the per-slot kernel times of one more call (zmi_ctx_get_timing: 5 = plan
               and history, 3 = decode, 6 = resolve, 4 = the decode's status step, 7 = got / status and the trimmed copy),
  yardstick    zmi_inflate_batch_dev over the same decoded volume cut into independent gzip members of equal size.
Warm-up first, HIP events, median of --reps; the ranges' bytes are compared with the data once.  Prints one JSON line and writes it to
--out (default profiles/inflate_ranges.json)."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS = {3: "decode", 4: "status", 5: "plan_history", 6: "resolve", 7: "finish_copy"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=4096)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--span", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_ranges.json"))
    a = ap.parse_args()
    import numpy as np
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
    s, idx = e.deflate_stream(data, level=a.level, wrap=WRAP_GZIP, piece_bytes=B, index=True)
    stream, cuts = s.clone(), (idx[:-1] * 8).clone()
    del s, idx
    back = torch.empty(raw, dtype=torch.uint8, device=e.device)

    def timed(f):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), r

    # ---- the cost of keeping the index ----
    plain = lambda: e.inflate_plain_stream(stream, wrap=WRAP_GZIP, bit_index=cuts, piece_out_max=B, out=back)
    indexed = lambda: e.inflate_stream_indexed(stream, wrap=WRAP_GZIP, bit_cuts=cuts, span=a.span, piece_out_max=B, out=back)
    ms = {"plain": [], "indexed": []}
    index = None
    for rep in range(a.reps + 1):                    # the first round is the warm-up and the check
        for k, f in (("plain", plain), ("indexed", indexed)):
            back.fill_(0)
            t, r = timed(f)
            if rep:
                ms[k].append(t)
            else:
                assert torch.equal(back, data), k
            if k == "indexed":
                index = r[2]
    mp, mi = statistics.median(ms["plain"]), statistics.median(ms["indexed"])
    res = {"probe": "inflate_ranges", "shards": n, "shard_bytes": B, "level": a.level, "wrap": "gzip", "reps": a.reps, "span": a.span,
           "device": torch.cuda.get_device_name(0), "stream_bytes": int(stream.numel()), "points": index.n_points, "max_gap": index.max_gap,
           "index_bytes": index.n_points * (16 + 32768),
           "plain_ms_median": round(mp, 3), "indexed_ms_median": round(mi, 3), "index_cost_ms": round(mi - mp, 3),
           "plain_ms_spread": round(max(ms["plain"]) - min(ms["plain"]), 3), "plain_gib_s": round(raw / 2**30 / (mp / 1e3), 2)}
    del back

    # ---- range reads, and the batch decoder over the same decoded volume ----
    offs = np.array(index.out.tolist(), dtype=np.int64)
    for name, count, length in (("64KiB_x4096", 4096, 64 << 10), ("1MiB_x256", 256, 1 << 20)):
        assert length < raw
        r = random.Random(count)
        los = [r.randrange(0, raw - length) for _ in range(count)]
        k = np.searchsorted(offs[:-1], np.array(los), side="right") - 1
        decoded = int((np.array(los) - offs[k]).sum()) + count * length
        lo = torch.tensor(los, dtype=torch.int64, device=e.device)
        ln = torch.full((count,), length, dtype=torch.int32, device=e.device)
        out = torch.empty((count, length), dtype=torch.uint8, device=e.device)
        read = lambda: e.read_ranges(stream, index, lo, ln, out=out, max_len=length)
        times = []
        for rep in range(a.reps + 1):
            t, (_, got, st) = timed(read)
            if rep:
                times.append(t)
            else:
                assert st.tolist() == [0] * count and got.tolist() == [length] * count
                for i in range(0, count, max(1, count // 64)):
                    assert torch.equal(out[i], data[los[i]:los[i] + length]), i
        sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)   # (drops what was recorded before)
        L.zmi_ctx_set_timing(e._ctx, 1)
        read()
        torch.cuda.synchronize()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)
        L.zmi_ctx_set_timing(e._ctx, 0)
        med = statistics.median(times)
        # the yardstick: `count` independent gzip members that decode to the same volume
        # (never more than the data holds: a small --shards decodes the same bytes many times over)
        m = max(1, min(decoded // count, raw // count))
        assert count * m <= raw
        moff, mln = uniform_layout(count, m, e.device)
        slots, olen, dst = e.deflate_batch(data, moff, mln, m, level=a.level, wrap=WRAP_GZIP)
        assert int((dst != 0).sum().item()) == 0
        coff = torch.arange(count, dtype=torch.int64, device=e.device) * slots.stride(0)
        mback = torch.empty(count * m, dtype=torch.uint8, device=e.device)
        mcap = torch.full((count,), m, dtype=torch.int32, device=e.device)
        btimes = []
        for rep in range(a.reps + 1):
            t, _ = timed(lambda: e.inflate_batch(slots, coff, olen, mback, moff, mcap, wrap=WRAP_GZIP))
            if rep:
                btimes.append(t)
            else:
                assert torch.equal(mback, data[:count * m])
        bmed = statistics.median(btimes)
        res[name] = {"ms_median": round(med, 3), "ms_spread": round(max(times) - min(times), 3),
                     "delivered_gib_s": round(count * length / 2**30 / (med / 1e3), 2), "decoded_bytes": decoded,
                     "decoded_gib_s": round(decoded / 2**30 / (med / 1e3), 2), "slots_ms": {SLOTS[i]: round(sums[i], 3) for i in SLOTS},
                     "batch_members_bytes": count * m, "batch_members_ms_median": round(bmed, 3), "batch_members_gib_s": round(count * m / 2**30 / (bmed / 1e3), 2)}
        del out, slots, mback
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
