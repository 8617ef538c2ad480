"""What writing PNG images on the MI355X costs, stage by stage: zmi_png_encode_dev (the forward filter / Adler-32,
CRC-32 and the folds / match search, parse, encode / layout, places and pack / the files' fixed bytes) from the context's event timing,
against the yardstick -- what a caller had before, with the host filtering left out in its favour: zmi_deflate_batch_dev(ZMI_WRAP_ZLIB)
on the same, already filtered scanlines with hand-made tables, zmi_checksum_batch_dev over the outputs (the IDAT CRC-32) and
zmi_pack_slab_dev.

Images: gen_shards data as pixels, level 6, adaptive filter, piece_bytes 1 MiB.  Workloads: 4096 x 256x256 RGB, 256 x 2048x2048 RGBA,
one 8192x8192 RGB image -- the reader's cases (tools/gpu_png_probe.py).  Every file is decoded back by Engine.png_decode and compared
with the pixels.  The ratio is recorded with strategy 0 and with strategy 1 (Z_FILTERED).  One JSON line per run; the committed one is
profiles/png_write.json.

    python tools/gpu_png_write_probe.py [--small 4096] [--medium 256] [--large 1] [--reps 5] [--out profiles/png_write.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_ZLIB, PNG_IMAGE_BYTES   # noqa: E402

SLOTS = {"checksums": 0, "match_search": 1, "encode": 2, "filter": 3, "files": 4, "parse": 5, "framing": 7}
HBM_TB_S = 6.29         # measured read + write rate of one MI355X (the microarchitecture guide)


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


def measure(e, n, w, h, colour, reps):
    dev = e.device
    ch = 3 if colour == 2 else 4
    rb, size, ssz = w * ch, w * ch * h, (1 + w * ch) * h
    total = n * size
    pixels = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    table = np.zeros((n, PNG_IMAGE_BYTES), dtype=np.uint8)
    table.view("<u4")[:, 0], table.view("<u4")[:, 1] = w, h
    table[:, 8], table[:, 9] = 8, colour
    table = torch.from_numpy(table).to(dev)
    offs = torch.arange(n, dtype=torch.int64, device=dev) * size
    lens = torch.full((n,), size, dtype=torch.int32, device=dev)
    images = (pixels, offs, lens, table)
    out = torch.empty(e.png_bound(n, n * ssz, 1 << 20, 1, 6), dtype=torch.uint8, device=dev)
    res = {"images": n, "width": w, "height": h, "channels": ch, "pixel_bytes": total, "scanline_bytes": n * ssz}

    def encode(strategy=0):
        return e.png_encode(images, level=6, strategy=strategy, out=out, scan_bytes=n * ssz)

    def check(strategy):
        _, off, ln, st = encode(strategy)
        assert bool((st == 0).all()), "a status is not 0"
        batch = e.png_headers(out, off[:n], ln)
        assert bool(batch.readable.all())
        back = torch.empty(total, dtype=torch.uint8, device=dev)
        _, _, _, dst = e.png_decode(None, batch, out=back, align=1)
        assert bool((dst == 0).all()) and torch.equal(back, pixels), "the files do not decode to the pixels"
        return int(off[n].item()), batch

    files1, _ = check(1)
    files0, batch = check(0)
    res["file_bytes"], res["ratio"] = files0, round(total / files0, 4)
    res["file_bytes_filtered_strategy"], res["ratio_filtered_strategy"] = files1, round(total / files1, 4)
    res["encode_ms"] = stages(e, encode, reps)
    med, spread = wall(encode, reps)
    res["encode"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)}
    f_ms = res["encode_ms"]["filter"]
    bound_ms = (total + n * ssz) / (HBM_TB_S * 1e12) * 1e3
    res["filter"] = {"ms": f_ms, "share": round(f_ms / med, 4), "gb_s_of_pixels": round(total / f_ms / 1e-3 / 1e9, 1),
                     "hbm_bound_ms": round(bound_ms, 4), "times_the_bound": round(f_ms / bound_ms, 2)}
    # the yardstick: the batch encoder on the filtered scanlines (inflated here from the files just written), the CRC-32 of its
    # outputs, the pack
    scan = torch.empty(n * ssz, dtype=torch.uint8, device=dev)
    soff = torch.arange(n, dtype=torch.int64, device=dev) * ssz
    scap = torch.full((n,), ssz, dtype=torch.int32, device=dev)
    zoff = (batch.offsets + 41).contiguous()
    zlen = (batch.lengths - 41 - 16).to(torch.int32).contiguous()
    olen, ost = e.inflate_batch(out, zoff, zlen, scan, soff, scap, wrap=WRAP_ZLIB)
    assert bool((ost == 0).all()) and bool((olen == ssz).all())
    share = scan.view(n * h, 1 + rb)[:, 0].to(torch.int64).bincount(minlength=5).tolist()
    res["filter_share"] = [round(x / (n * h), 4) for x in share]
    stride = e.deflate_bound(ssz, WRAP_ZLIB)
    slots = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    ylen, yst = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    slab = torch.empty(out.numel(), dtype=torch.uint8, device=dev)
    yoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    crc = torch.zeros(n, dtype=torch.int32, device=dev)
    slot_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    try:
        def yard():
            e.deflate_batch(scan, soff, scap, ssz, level=6, wrap=WRAP_ZLIB, out=slots, out_len=ylen, status=yst)
            e.checksums(slots.view(-1), slot_off, ylen, adler=False, crc=True, out_crc=crc)
            e.pack_slab(slots, ylen, slab=slab, offsets=e.scan_sizes(ylen, out=yoff))

        med_y, spread_y = wall(yard, reps)
        assert bool((yst == 0).all())
        res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "bytes": int(yoff[n].item())}
        res["encode_over_yardstick"] = round(med / med_y, 4)
    except RuntimeError as err:                  # (one shard of hundreds of MB may not fit the batch encoder's scratch)
        res["yardstick"] = {"error": str(err)[:200]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=4096)
    ap.add_argument("--medium", type=int, default=256)
    ap.add_argument("--large", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_png_write_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "png_write", "level": 6, "filter": "adaptive", "piece_bytes": 1 << 20, "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "filter_tile": int(L.zmi_png_filter_tile()), "hbm_tb_s": HBM_TB_S}
    if a.small:
        line["small"] = measure(e, a.small, 256, 256, 2, a.reps)
    if a.medium:
        line["medium"] = measure(e, a.medium, 2048, 2048, 6, a.reps)
    if a.large:
        line["large"] = measure(e, a.large, 8192, 8192, 2, a.reps)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
