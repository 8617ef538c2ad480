#!/usr/bin/env python3
"""Single-stream inflate through the block scan against the marker path, on the same bytes in one process: --shards x 1 MiB generated
shards at level 6, gzip, from Engine.deflate_stream, as
  find_blocks   zmi_stream_find_blocks_dev alone (default min_gap),
  blocks        Engine.inflate_plain_stream (zmi_inflate_stream_bits_dev) with those proposals given,
  markers       Engine.inflate_stream (zmi_inflate_stream_dev) with the stream's own piece index,
alternating, timed with HIP events, median of --reps; every result is compared with the input once.  Per-stage kernel times of one
more call of each path come from the context's timers (zmi_ctx_get_timing: decode = kernel 3, symbolic resolve = 6, window scan = 5,
substitute + offsets = 7, checksums = 0, header / setup / verification / trailer = 4; the scan of find_blocks is recorded under 4).
Then one true ordinary stream: --plain-mib MiB of the same data through the host's zlib at level 6, one gzip member without a flush
point.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = {0: "checksum", 3: "decode", 4: "verify", 5: "window_scan", 6: "symbolic_resolve", 7: "substitute_offsets"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=16384)
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-mib", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from zlib_rs_amd import _lib
    from zlib_rs_amd.engine import Engine, WRAP_GZIP
    e = Engine(0)
    L = _lib.lib()
    L.zmi_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.zmi_ctx_get_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]

    def timed(f):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = f()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), r

    def stages(f):
        sums, counts = (C.c_double * 8)(), (C.c_uint32 * 8)()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)   # (drops what was recorded before)
        L.zmi_ctx_set_timing(e._ctx, 1)
        f()
        torch.cuda.synchronize()
        L.zmi_ctx_get_timing(e._ctx, sums, counts)
        L.zmi_ctx_set_timing(e._ctx, 0)
        return {STAGES[i]: round(sums[i], 3) for i in STAGES}

    def measure(s, data, forms, res, tag):
        raw = data.numel()
        back = torch.empty(raw, dtype=torch.uint8, device=e.device)
        ms = {k: [] for k in forms}
        pom = {}
        for rep in range(a.reps + 1):                # the first round is the warm-up and the check
            for k, f in forms.items():
                back.fill_(0)
                t, _ = timed(lambda: f(back, pom.get(k)))   # (later rounds start at the piece_out_max the first one ended with)
                if rep:
                    ms[k].append(t)
                else:
                    assert torch.equal(back, data), k
                    pom[k] = e.last_piece_out_max
        for k, f in forms.items():
            med = statistics.median(ms[k])
            res[tag + k] = {"ms_median": round(med, 3), "gib_s": round(raw / 2**30 / (med / 1e3), 2), "piece_out_max": pom[k],
                            "stages_ms": stages(lambda: f(back, pom[k]))}

    n, B = a.shards, a.shard_bytes
    data = e.gen_shards(n, B)
    s, idx = e.deflate_stream(data, level=a.level, wrap=WRAP_GZIP, piece_bytes=B, index=True)
    s, idx = s.clone(), idx[:-1].clone()
    torch.cuda.synchronize()
    res = {"probe": "stream_inflate_blocks_dev", "shards": n, "shard_bytes": B, "level": a.level, "wrap": "gzip", "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "stream_bytes": int(s.numel())}
    t = [timed(lambda: e.find_blocks(s, wrap=WRAP_GZIP)) for _ in range(a.reps + 1)]
    cuts = t[0][1]
    med = statistics.median(x[0] for x in t[1:])
    res["find_blocks"] = {"ms_median": round(med, 3), "gib_s_of_input": round(s.numel() / 2**30 / (med / 1e3), 2), "pieces": int(cuts.numel()),
                          "stages_ms": stages(lambda: e.find_blocks(s, wrap=WRAP_GZIP))}
    res["marker_pieces"] = int(idx.numel())
    measure(s, data, {"blocks": lambda out, pom: e.inflate_plain_stream(s, wrap=WRAP_GZIP, bit_index=cuts, piece_out_max=pom, out=out),
                      "markers": lambda out, pom: e.inflate_stream(s, wrap=WRAP_GZIP, index=idx, piece_out_max=pom or B, out=out)}, res, "stream_")
    res["blocks_vs_markers"] = round(res["stream_blocks"]["gib_s"] / res["stream_markers"]["gib_s"], 3)
    res["scan_vs_decode_stage"] = round(res["find_blocks"]["ms_median"] / res["stream_blocks"]["stages_ms"]["decode"], 3)
    if a.plain_mib:
        part = data[:a.plain_mib << 20].clone()
        del data, s, idx, cuts
        torch.cuda.empty_cache()
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        z = c.compress(bytes(part.cpu().numpy())) + c.flush()
        dev = torch.from_numpy(np.frombuffer(z, dtype=np.uint8).copy()).to(e.device)
        t = [timed(lambda: e.find_blocks(dev, wrap=WRAP_GZIP)) for _ in range(a.reps + 1)]
        pc = t[0][1]
        res["plain"] = {"mib": a.plain_mib, "stream_bytes": len(z), "marker_cuts": int(e.find_cuts(dev, wrap=WRAP_GZIP).numel()),
                        "pieces": int(pc.numel()), "find_blocks_ms_median": round(statistics.median(x[0] for x in t[1:]), 3)}
        measure(dev, part, {"blocks": lambda out, pom: e.inflate_plain_stream(dev, wrap=WRAP_GZIP, bit_index=pc, piece_out_max=pom, out=out),
                            "scan_and_blocks": lambda out, pom: e.inflate_plain_stream(dev, wrap=WRAP_GZIP, piece_out_max=pom, out=out)}, res, "plain_")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
