"""What writing a tiled Deflate TIFF on the MI355X costs, stage by stage: zmi_tiff_write_dev (the forward
predictor / Adler-32 and the fold / match search, parse, encode / the piece table, places and pack / the file's fixed bytes) from the
context's event timing, against the yardstick -- what a caller had before, with the predictor and the framing on the host left out in
its favour: zmi_deflate_batch_dev(ZMI_WRAP_ZLIB) on the same, already predicted segments with hand-made tables.  The predict kernel
alone is reported in bytes read plus bytes written per second beside a device copy of the same bytes; the write, the yardstick and
the copy take turns inside every repeat.

Pages: gen_shards data as samples, level 6, piece_bytes 1 MiB, BigTIFF, the dense input form (tile k at k * its size).  Workloads: 4096
tiles of 256 x 256 RGB8 with predictor 2, 1024 tiles of 512 x 512 float32 with predictor 3 -- the reader's cases
(tools/gpu_tiff_probe.py).  Every file is read back by Engine.tiff_read and compared with the samples.  One JSON line per run; the
committed one is profiles/tiff_write.json.

    python tools/gpu_tiff_write_probe.py [--rgb 4096] [--float 1024] [--reps 5] [--out profiles/tiff_write.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_ZLIB   # noqa: E402

SLOTS = {"checksums": 0, "match_search": 1, "encode": 2, "predict": 3, "file": 4, "parse": 5, "framing": 7}


def timing(e):
    sums, cnts = (C.c_double * 8)(), (C.c_uint32 * 8)()
    e.L.zmi_ctx_get_timing(e._ctx, sums, cnts)
    return list(sums), list(cnts)


def wall(fns, reps):
    """[(median, spread)] in ms of `reps` calls of every function between device events, after one warm-up each; the functions take
    turns inside every repeat, so that what is compared runs under the same clocks and the same state of the caches"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = []
    for m in ms:
        m.sort()
        out.append((m[len(m) // 2], m[-1] - m[0]))
    return out


def stages(e, fn, reps):
    fn()
    torch.cuda.synchronize()
    e.L.zmi_ctx_set_timing(e._ctx, 1)
    for _ in range(reps):
        fn()
    sums, _ = timing(e)
    e.L.zmi_ctx_set_timing(e._ctx, 0)
    return {k: round(sums[s] / reps, 4) for k, s in SLOTS.items()}


def measure(e, n, tile, samples, dtype, reps):
    dev = e.device
    side = int(round(n ** 0.5))
    assert side * side == n, "the tiles make a square page"
    sb = torch.empty(0, dtype=dtype).element_size()
    size = tile * tile * samples * sb
    total = n * size
    data = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    offs = torch.arange(n, dtype=torch.int64, device=dev) * size
    shape = (side * tile, side * tile, samples)
    kw = dict(tile=tile, level=6, piece_bytes=1 << 20, bigtiff=True)
    out = torch.empty(e.tiff_bound(shape, dtype, **kw), dtype=torch.uint8, device=dev)
    res = {"tiles": n, "tile": tile, "samples": samples, "sample_bytes": sb, "predictor": 3 if dtype.is_floating_point else 2, "page_bytes": total}

    def write():
        return e.tiff_write((data, offs, shape, dtype), out=out, **kw)

    _, file_len, seg_len, st = write()
    assert st.tolist() == [0] * (n + 1), "a status is not 0"
    file_len = int(file_len)
    tf = e.tiff_directory(out[:file_len])
    back, _, _, rst = e.tiff_read(None, tf, assemble=False, align=16)
    assert bool((rst == 0).all()) and torch.equal(back[:total], data), "the file does not read back to the samples"
    res["file_bytes"], res["ratio"] = file_len, round(total / file_len, 4)
    # the yardstick: the batch encoder on the predicted segments (inflated here from the file just written), hand-made tables; the
    # copy: the same bytes read and written once, the predict kernel's memory floor
    scan = torch.empty(total, dtype=torch.uint8, device=dev)
    copy = torch.empty(total, dtype=torch.uint8, device=dev)
    rec = tf.record(0)
    zoff = out[rec["offsets_pos"]:rec["offsets_pos"] + 8 * n].clone().view(torch.int64)
    zlen = out[rec["counts_pos"]:rec["counts_pos"] + 8 * n].clone().view(torch.int64).to(torch.int32)
    scap = torch.full((n,), size, dtype=torch.int32, device=dev)
    olen, ost = e.inflate_batch(out, zoff, zlen, scan, offs, scap, wrap=WRAP_ZLIB)
    assert bool((ost == 0).all()) and bool((olen == size).all())
    stride = e.deflate_bound(size, WRAP_ZLIB)
    slots = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    ylen, yst = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def yard():
        e.deflate_batch(scan, offs, scap, size, level=6, wrap=WRAP_ZLIB, out=slots, out_len=ylen, status=yst)

    res["write_ms"] = stages(e, write, reps)
    (med, spread), (med_y, spread_y), (c_med, c_spread) = wall([write, yard, lambda: copy.copy_(data)], reps)
    assert bool((yst == 0).all())
    res["write"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)}
    p_ms = res["write_ms"]["predict"]
    res["predict"] = {"ms": p_ms, "share": round(p_ms / med, 4), "gb_s_read_plus_written": round(2 * total / p_ms / 1e-3 / 1e9, 1),
                      "copy_ms_median": round(c_med, 4), "copy_ms_spread": round(c_spread, 4),
                      "copy_gb_s_read_plus_written": round(2 * total / c_med / 1e-3 / 1e9, 1), "time_over_copy": round(p_ms / c_med, 2)}
    res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "bytes": int(ylen.sum().item())}
    res["write_over_yardstick"] = round(med / med_y, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rgb", type=int, default=4096)
    ap.add_argument("--float", type=int, default=1024, dest="flt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_tiff_write_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "tiff_write", "level": 6, "piece_bytes": 1 << 20, "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "predict_tile": int(L.zmi_tiff_predict_tile())}
    if a.rgb:
        line["rgb8_256"] = measure(e, a.rgb, 256, 3, torch.uint8, a.reps)
    if a.flt:
        line["float32_512"] = measure(e, a.flt, 512, 1, torch.float32, a.reps)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
