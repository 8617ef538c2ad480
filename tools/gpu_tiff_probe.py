"""What reading a tiled Deflate TIFF on the MI355X costs, stage by stage: zmi_tiff_directory_dev and
zmi_tiff_read_dev (slot tables and plans / decode / resolve / unpredict / slot words) from the context's event timing, against two
yardsticks: the whole call against zmi_inflate_batch_dev(ZMI_WRAP_ZLIB) on the same segments with hand-made true tables, which parses
nothing and unpredicts nothing; the unpredict's event slot against a plain device copy of the same number of bytes, its memory floor.

Files: gen_shards data as pixels, one BigTIFF page of square tiles, predicted on the host, zlib level 6.  Workloads: 4096 tiles of
256 x 256 RGB uint8 with predictor 2; 1024 tiles of 512 x 512 float32 with predictor 3.  Every result is compared with the pixels.
One JSON line per run; the committed one is profiles/tiff_read.json.

    python tools/gpu_tiff_probe.py [--rgb 4096] [--float 1024] [--reps 5] [--out profiles/tiff_read.json]
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_ZLIB   # noqa: E402

SLOTS = {"adler": 0, "unpredict": 2, "decode": 3, "words": 4, "plan": 5, "resolve": 6, "copies": 7}


def predict_tile(t, sb, samples, pred):
    """t uint8 [rows, seg_w * samples * sb], little-endian samples -> the bytes handed to the compressor (TIFF 6.0 section 14; Technical
    Note 3)"""
    rows = t.shape[0]
    if pred == 2:
        x = t.view("<u%d" % sb).reshape(rows, -1, samples)
        d = x.copy()
        d[:, 1:] = x[:, 1:] - x[:, :-1]
        return d.tobytes()
    n = t.shape[1] // sb
    planes = t.reshape(rows, n, sb)[:, :, ::-1].transpose(0, 2, 1).reshape(rows, -1, samples)      # most significant plane first
    q = planes.copy()
    q[:, 1:] = planes[:, 1:] - planes[:, :-1]
    return q.tobytes()


def craft(host, side, tile, samples, sb, fmt, pred):
    """host uint8 [side, side * samples * sb] -> (a little-endian BigTIFF of one tiled page, the tiles' offsets, their byte counts)"""
    across = side // tile
    pb = samples * sb

    def one(k):
        ty, tx = divmod(k, across)
        t = np.ascontiguousarray(host[ty * tile:(ty + 1) * tile, tx * tile * pb:(tx + 1) * tile * pb])
        return zlib.compress(predict_tile(t, sb, samples, pred), 6)

    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        segs = list(pool.map(one, range(across * across)))
    out = bytearray(b"II" + struct.pack("<HHHQ", 43, 8, 0, 0))
    offs, cnts = [], []
    for s in segs:
        offs.append(len(out))
        cnts.append(len(s))
        out += s
    n = len(segs)
    at_off = len(out)
    out += struct.pack("<%dQ" % n, *offs)
    at_cnt = len(out)
    out += struct.pack("<%dQ" % n, *cnts)
    ent = [(256, 4, 1, side), (257, 4, 1, side), (258, 3, samples, None), (259, 3, 1, 8), (262, 3, 1, 2 if samples == 3 else 1),
           (277, 3, 1, samples), (284, 3, 1, 1), (317, 3, 1, pred), (322, 4, 1, tile), (323, 4, 1, tile), (324, 16, n, at_off),
           (325, 16, n, at_cnt), (339, 3, samples, None)]
    struct.pack_into("<Q", out, 8, len(out))
    out += struct.pack("<Q", len(ent))
    for tag, typ, cnt, val in ent:
        field = struct.pack("<Q", val) if val is not None else struct.pack("<4H", *([8 * sb if tag == 258 else fmt] * samples + [0] * (4 - samples)))
        out += struct.pack("<HHQ", tag, typ, cnt) + field
    out += struct.pack("<Q", 0)
    return bytes(out), offs, cnts


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


def measure(e, n_tiles, tile, samples, sb, fmt, pred, reps):
    L, ctx, dev = e.L, e._ctx, e.device
    across = int(round(n_tiles ** 0.5))
    assert across * across == n_tiles
    side, pb = across * tile, samples * sb
    total = side * side * pb
    pixels = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    torch.cuda.synchronize()
    blob, offs, cnts = craft(pixels.cpu().numpy().reshape(side, side * pb), side, tile, samples, sb, fmt, pred)
    res = {"tiles": n_tiles, "tile": tile, "samples": samples, "sample_bytes": sb, "predictor": pred, "pixel_bytes": total, "file_bytes": len(blob),
           "row_tile": int(L.zmi_tiff_row_tile())}
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    tf = e.tiff_directory(data)
    assert bool(tf.readable.all()) and tf.grid(0) == (across, across)
    dm, ds = wall(lambda: e.tiff_directory(data), reps)
    res["directory"] = {"ms_median": round(dm, 4), "ms_spread": round(ds, 4)}
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    img, st = e.tiff_read(None, tf, out=out)
    assert bool((st == 0).all()) and torch.equal(out, pixels), "the assembled image is wrong"
    dense, off, ln, st = e.tiff_read(None, tf, assemble=False, align=1)
    want = pixels.view(across, tile, across, tile * pb).permute(0, 2, 1, 3).contiguous().view(-1)
    assert bool((st == 0).all()) and torch.equal(dense, want), "the dense tiles are wrong"
    del dense, want
    res["read_ms"] = stages(e, lambda: e.tiff_read(None, tf, out=out), reps)
    med, spread = wall(lambda: e.tiff_read(None, tf, out=out), reps)
    res["read"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)}
    res["unpredict_share"] = round(res["read_ms"]["unpredict"] / med, 4)
    res["unpredict_gib_s"] = round(total / res["read_ms"]["unpredict"] / 1e-3 / 2 ** 30, 2)
    # the unpredict's floor: one read and one write of the same number of bytes
    src = torch.empty_like(out)
    cm, cs = wall(lambda: src.copy_(out), reps)
    res["copy"] = {"ms_median": round(cm, 4), "ms_spread": round(cs, 4), "gib_s": round(total / cm / 1e-3 / 2 ** 30, 2)}
    res["unpredict_over_copy"] = round(res["read_ms"]["unpredict"] / cm, 3)
    del src
    # the yardstick: the batch decoder on the same segments where they stand, true tables
    seg = tile * tile * pb
    in_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    in_len = torch.tensor(cnts, dtype=torch.int32, device=dev)
    cap = torch.full((n_tiles,), seg, dtype=torch.int32, device=dev)
    ooff = torch.arange(n_tiles, dtype=torch.int64, device=dev) * seg
    olen, ost = torch.zeros(n_tiles, dtype=torch.int32, device=dev), torch.zeros(n_tiles, dtype=torch.int32, device=dev)
    L.zmi_ctx_set_inflate_out_limit(ctx, total + (1 << 16))

    def yard():
        L.zmi_inflate_batch_dev(ctx, data.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n_tiles, WRAP_ZLIB, out.data_ptr(), ooff.data_ptr(),
                                cap.data_ptr(), olen.data_ptr(), ost.data_ptr(), None)

    med_y, spread_y = wall(yard, reps)
    assert bool((ost == 0).all()) and bool((olen == seg).all())
    L.zmi_ctx_set_inflate_out_limit(ctx, 0)
    res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "gib_s": round(total / med_y / 1e-3 / 2 ** 30, 2)}
    res["read_over_yardstick"] = round(med / med_y, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rgb", type=int, default=4096)
    ap.add_argument("--float", type=int, default=1024, dest="flt")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_tiff_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "tiff_read", "level": 6, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    if a.rgb:
        line["rgb8_predictor2"] = measure(e, a.rgb, 256, 3, 1, 1, 2, a.reps)
    if a.flt:
        line["float32_predictor3"] = measure(e, a.flt, 512, 1, 4, 3, 3, a.reps)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
