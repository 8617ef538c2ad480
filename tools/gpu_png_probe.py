"""What reading PNG images on the MI355X costs, stage by stage: zmi_png_headers_dev and zmi_png_decode_dev (slot
tables and plans / the walk: chunk CRC-32 and gather / decode / resolve / unfilter / slot words) from the context's event timing,
against the yardstick -- the existing path on the same IDAT streams: zmi_inflate_batch_dev(ZMI_WRAP_ZLIB) with hand-made true tables,
which parses nothing and unfilters nothing.

Images: gen_shards data as pixels, filtered on the host per row by the minimum sum of absolute differences (what libpng's adaptive
heuristic does), zlib level 6, one IDAT per file (--idat N cuts the stream into chunks of N bytes).  Workloads: 4096 x 256x256 RGB,
256 x 2048x2048 RGBA, one 8192x8192 RGB image; the last one also with chain splitting off (ZMI_PNG_SPLIT=0).  One JSON line per run;
the committed one is profiles/png_read.json.

    python tools/gpu_png_probe.py [--small 4096] [--medium 256] [--large 1] [--reps 5] [--idat 0] [--out profiles/png_read.json]
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import struct
import sys
import zlib

os.environ.setdefault("ZMI_TUNING", "1")        # ZMI_PNG_SPLIT below
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_ZLIB   # noqa: E402

SLOTS = {"crc_adler": 0, "unfilter": 2, "decode": 3, "words": 4, "plan": 5, "resolve": 6}


def filter_image(px, bpp):
    """px uint8 [H, rb] -> (scanlines uint8 [H, 1 + rb], filter types [H]): per row the type of the smallest sum of absolute
    differences, the bytes taken as signed (section 12.8 of the specification)"""
    H, rb = px.shape
    x = px.astype(np.int16)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)          # [5, H, rb]
    cost = np.abs(cand.view(np.int8).astype(np.int16)).sum(axis=2)                              # [5, H]
    types = cost.argmin(axis=0).astype(np.uint8)
    scan = np.empty((H, 1 + rb), dtype=np.uint8)
    scan[:, 0] = types
    scan[:, 1:] = cand[types, np.arange(H)]
    return scan, types


def chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data))


def craft(px, w, h, colour, bpp, idat):
    scan, types = filter_image(px, bpp)
    stream = zlib.compress(scan.tobytes(), 6)
    head = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0))
    pieces = [stream] if not idat else [stream[i:i + idat] for i in range(0, len(stream), idat)]
    body = b"".join(chunk(b"IDAT", p) for p in pieces)
    return head + body + chunk(b"IEND", b""), types, len(head), len(stream), len(pieces)


def chains(types, split=True):
    """the unfilter's chains of an image (csrc/png_kernels.h) -> (number of chains, 64-row bands they take, bands of the longest)"""
    H = len(types)
    starts = [0]
    if split:
        for band in range(1, (H + 63) // 64):
            rows = np.nonzero(types[band * 64:band * 64 + 64] <= 1)[0]
            if rows.size:
                starts.append(band * 64 + int(rows[0]))
    ends = starts[1:] + [H]
    per = [(e - s + 63) // 64 for s, e in zip(starts, ends)]
    return len(starts), sum(per), max(per)


def band_steps(rb, bpp, strip):
    """steps one band of 64 rows takes: every strip of the scanline is drained, pixels + 63"""
    per = strip // bpp * bpp
    return sum(min(per, rb - c0) // bpp + 63 for c0 in range(0, rb, per))


def timing(e):
    sums, cnts = (C.c_double * 8)(), (C.c_uint32 * 8)()
    e.L.zmi_ctx_get_timing(e._ctx, sums, cnts)
    return list(sums), list(cnts)


def wall(fn, reps):
    """median and spread (ms) of `reps` calls between device events, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[-1] - ms[0]


def stages(e, fn, reps):
    fn()
    torch.cuda.synchronize()
    e.L.zmi_ctx_set_timing(e._ctx, 1)
    for _ in range(reps):
        fn()
    sums, _ = timing(e)
    e.L.zmi_ctx_set_timing(e._ctx, 0)
    return {k: round(sums[s] / reps, 4) for k, s in SLOTS.items()}


def measure(e, n, w, h, colour, reps, idat, unsplit=False):
    L, ctx, dev = e.L, e._ctx, e.device
    strip = int(L.zmi_png_strip())
    ch = 3 if colour == 2 else 4
    rb, size = w * ch, w * ch * h
    total = n * size
    pixels = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    torch.cuda.synchronize()
    host = pixels.cpu().numpy().reshape(n, h, rb)
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        made = list(pool.map(lambda i: craft(host[i], w, h, colour, ch, idat), range(n)))
    blobs = [m[0] for m in made]
    geo = [chains(m[1]) for m in made]
    res = {"images": n, "width": w, "height": h, "channels": ch, "pixel_bytes": total, "file_bytes": sum(len(x) for x in blobs),
           "idat_chunks_per_image": made[0][4], "chains": sum(g[0] for g in geo),
           "lane_utilisation": round(n * h / (64.0 * sum(g[1] for g in geo)), 4),
           "filter_share": [round(float(np.mean(np.concatenate([m[1] for m in made]) == t)), 4) for t in range(5)],
           "serial_steps_longest_chain": max(g[2] for g in geo) * band_steps(rb, ch, strip)}
    b = e.png_headers(blobs)
    assert bool(b.readable.all())
    hm, hs = wall(lambda: e.png_headers(b.data, b.offsets, b.lengths), reps)
    res["headers"] = {"ms_median": round(hm, 4), "ms_spread": round(hs, 4)}
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    _, off, ln, st = e.png_decode(None, b, out=out, align=1)
    assert bool((st == 0).all()) and torch.equal(out, pixels), "decode is wrong"
    res["decode_ms"] = stages(e, lambda: e.png_decode(None, b, out=out, align=1), reps)
    no_crc = stages(e, lambda: e.png_decode(None, b, out=out, align=1, check_crc=False), reps)
    res["decode_ms"]["adler_alone"] = no_crc["crc_adler"]
    med, spread = wall(lambda: e.png_decode(None, b, out=out, align=1), reps)
    res["decode"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)}
    res["unfilter_share"] = round(res["decode_ms"]["unfilter"] / med, 4)
    res["unfilter_gib_s"] = round(total / res["decode_ms"]["unfilter"] / 1e-3 / 2 ** 30, 2)
    if unsplit:
        os.environ["ZMI_PNG_SPLIT"] = "0"
        out.zero_()
        _, _, _, st = e.png_decode(None, b, out=out, align=1)
        assert bool((st == 0).all()) and torch.equal(out, pixels), "decode without splitting is wrong"
        one = stages(e, lambda: e.png_decode(None, b, out=out, align=1), reps)
        med1, spread1 = wall(lambda: e.png_decode(None, b, out=out, align=1), reps)
        del os.environ["ZMI_PNG_SPLIT"]
        g1 = [chains(m[1], split=False) for m in made]
        res["unsplit"] = {"ms_median": round(med1, 3), "ms_spread": round(spread1, 3), "unfilter_ms": one["unfilter"], "chains": sum(g[0] for g in g1),
                          "serial_steps_longest_chain": max(g[2] for g in g1) * band_steps(rb, ch, strip)}
    # the yardstick: the batch decoder on the same streams where they stand (with --idat: gathered on the host), true tables
    if idat:
        streams = [zlib.compress(filter_image(host[i], ch)[0].tobytes(), 6) for i in range(n)]
        zdata = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()).to(dev)
        lens = np.array([len(s) for s in streams], dtype=np.int64)
        in_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).to(dev)
    else:
        zdata = b.data
        lens = np.array([m[3] for m in made], dtype=np.int64)
        in_off = (b.offsets + torch.tensor([m[2] + 8 for m in made], dtype=torch.int64, device=dev)).contiguous()
    in_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    ssz = (1 + rb) * h
    scan = torch.empty(n * ssz, dtype=torch.uint8, device=dev)
    cap = torch.full((n,), ssz, dtype=torch.int32, device=dev)
    ooff = torch.arange(n, dtype=torch.int64, device=dev) * ssz
    olen, ost = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    L.zmi_ctx_set_inflate_out_limit(ctx, n * ssz + (1 << 16))

    def yard():
        L.zmi_inflate_batch_dev(ctx, zdata.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, WRAP_ZLIB, scan.data_ptr(), ooff.data_ptr(),
                                cap.data_ptr(), olen.data_ptr(), ost.data_ptr(), None)

    med_y, spread_y = wall(yard, reps)
    assert bool((ost == 0).all()) and bool((olen == ssz).all())
    L.zmi_ctx_set_inflate_out_limit(ctx, 0)
    res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "gib_s": round(n * ssz / med_y / 1e-3 / 2 ** 30, 2)}
    res["decode_over_yardstick"] = round(med / med_y, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--medium", type=int, default=256)
    ap.add_argument("--large", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--idat", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_png_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "png_read", "level": 6, "reps": a.reps, "idat": a.idat, "device": torch.cuda.get_device_name(0), "strip": int(L.zmi_png_strip())}
    if a.small:
        line["small"] = measure(e, a.small, 256, 256, 2, a.reps, a.idat)
    if a.medium:
        line["medium"] = measure(e, a.medium, 2048, 2048, 6, a.reps, a.idat)
    if a.large:
        line["large"] = measure(e, a.large, 8192, 8192, 2, a.reps, a.idat, unsplit=True)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
