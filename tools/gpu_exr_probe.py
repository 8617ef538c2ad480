"""What reading OpenEXR files with ZIP compression on the MI355X costs, stage by stage: zmi_exr_headers_dev and
zmi_exr_read_dev (tables and plans / decode / resolve / raw copies / block sums, scan and unzip / slot words) from the context's event
timing, against two yardsticks: the whole call against zmi_inflate_batch_dev(ZMI_WRAP_ZLIB) on the same chunks with hand-made true
tables, which parses nothing and unzips nothing; the unzip's event slot against a plain device copy of the same number of bytes, its
memory floor.

Files: gen_shards data as pixels (the planes of the region as they stand), the predictor and the interleave done on the host, zlib
level 6.  Workloads: 64 frames of 2048 x 1080 RGBA HALF in chunks of 16 scanlines; one 4096 x 4096 RGBA HALF (256 chunks of 512 KiB: what
the block sums are for); 4096 tiles of 256 x 256 FLOAT in one file.  Every result is compared with the pixels.  One JSON line per run;
the committed one is profiles/exr_read.json.

--compression pxr24 crafts the same workloads with compression 5: the PXR24 forward on the host, the stream's
length m in place of n in the yardstick's tables, the undo kernel in the unzip's event slot, and FLOAT pixels compared as f24(..) << 8
in the chunks that are not stored raw.  The committed line is profiles/exr_pxr24.json.

    python tools/gpu_exr_probe.py [--compression zip] [--frames 64] [--big 4096] [--tiles 4096] [--reps 5] [--out profiles/exr_read.json]
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

SLOTS = {"adler": 0, "unzip": 2, "decode": 3, "words": 4, "plan": 5, "resolve": 6, "copies": 7}
HALF, FLOAT = 1, 2


def attr(name, type_, value):
    return name + b"\0" + type_ + b"\0" + struct.pack("<i", len(value)) + value


def zip_forward(raw):
    """raw bytes of a chunk (uint8 array) -> the bytes a ZIP writer hands to zlib"""
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int16)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 0xFF
    return d.astype(np.uint8).tobytes()


def f24(u):
    """the 32 bits of floats (uint32 array) -> their 24 bits (include/zmi355.h)"""
    s, e, m = u & np.uint32(0x80000000), u & np.uint32(0x7F800000), u & np.uint32(0x007FFFFF)
    rnd = ((e | m) + (m & np.uint32(0x80))) >> np.uint32(8)
    rnd = np.where(rnd >= 0x7F8000, (e | m) >> np.uint32(8), rnd)
    nan = (e >> np.uint32(8)) | (m >> np.uint32(8)) | ((m >> np.uint32(8)) == 0).astype(np.uint32)
    i = np.where(e == 0x7F800000, np.where(m != 0, nan, e >> np.uint32(8)), rnd)
    return ((s >> np.uint32(8)) | i).astype(np.uint32)


def pxr24_forward(rows, ptype):
    """rows uint8 [h, C, w * size] of one chunk -> (the bytes a PXR24 writer hands to zlib, the rows a reader returns for them)"""
    h, n_ch, _ = rows.shape
    v = np.ascontiguousarray(rows).view("<u2" if ptype == HALF else "<u4")
    back = rows
    if ptype == FLOAT:
        v = f24(v)
        back = (v << np.uint32(8)).view(np.uint8).reshape(rows.shape)
    p = 2 if ptype == HALF else 3
    d = v.astype(np.uint32)
    d[:, :, 1:] -= d[:, :, :-1].copy()
    planes = [((d >> np.uint32(8 * (p - 1 - j))) & np.uint32(255)).astype(np.uint8) for j in range(p)]
    return np.stack(planes, axis=2).tobytes(), back


def craft(planes, names, ptype, tile, pool, comp=3, lossy=None):
    """planes uint8 [C, H, W * size] -> (the file, the positions of the chunks' data, their sizes, their raw sizes or, under PXR24, the
    lengths their streams inflate to); lossy: under PXR24 the pixels a reader returns are written there"""
    n_ch, H, wb = planes.shape
    size = 2 if ptype == HALF else 4
    W = wb // size
    if tile:
        boxes = [(x0, y0, min(tile, W - x0), min(tile, H - y0)) for y0 in range(0, H, tile) for x0 in range(0, W, tile)]
    else:
        boxes = [(0, y0, W, min(16, H - y0)) for y0 in range(0, H, 16)]

    def one(box):
        x0, y0, w, h = box
        rows = np.ascontiguousarray(planes[:, y0:y0 + h, x0 * size:(x0 + w) * size].transpose(1, 0, 2))
        raw = rows.reshape(-1)
        if comp == 5:
            d, back = pxr24_forward(rows, ptype)
            packed = zlib.compress(d, 6)
            if len(packed) < raw.size and lossy is not None:
                lossy[:, y0:y0 + h, x0 * size:(x0 + w) * size] = back.transpose(1, 0, 2)
        else:
            packed = zlib.compress(zip_forward(raw), 6)
        return packed if len(packed) < raw.size else raw.tobytes()

    datas = list(pool.map(one, boxes))
    psize = size if comp != 5 or ptype == HALF else 3
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", ptype, 0, 1, 1) for n in names) + b"\0"
    head = bytes.fromhex("762f3101") + struct.pack("<I", 2 | (0x200 if tile else 0))
    head += attr(b"channels", b"chlist", chl) + attr(b"compression", b"compression", bytes([comp]))
    head += attr(b"dataWindow", b"box2i", struct.pack("<4i", 0, 0, W - 1, H - 1)) + attr(b"displayWindow", b"box2i", struct.pack("<4i", 0, 0, W - 1, H - 1))
    head += attr(b"lineOrder", b"lineOrder", b"\0") + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
    head += attr(b"screenWindowCenter", b"v2f", bytes(8)) + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
    if tile:
        head += attr(b"tiles", b"tiledesc", struct.pack("<IIB", tile, tile, 0))
    head += b"\0"
    at = len(head) + 8 * len(boxes)
    entries, pos, body = [], [], []
    for (x0, y0, w, h), data in zip(boxes, datas):
        hdr = struct.pack("<5i", x0 // tile, y0 // tile, 0, 0, len(data)) if tile else struct.pack("<2i", y0, len(data))
        entries.append(at)
        pos.append(at + len(hdr))
        body.append(hdr + data)
        at += len(hdr) + len(data)
    blob = head + struct.pack("<%dQ" % len(boxes), *entries) + b"".join(body)
    return blob, pos, [len(d) for d in datas], [w * h * n_ch * size for _, _, w, h in boxes], [w * h * n_ch * psize for _, _, w, h in boxes]


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


def measure(e, n_files, n_ch, H, W, ptype, tile, reps, pool, comp=3):
    L, ctx, dev = e.L, e._ctx, e.device
    size = 2 if ptype == HALF else 4
    region = n_ch * H * W * size
    total = n_files * region
    pixels = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    torch.cuda.synchronize()
    host = pixels.cpu().numpy().reshape(n_files, n_ch, H, W * size)
    names = ["A", "B", "G", "R"][:n_ch] if n_ch > 1 else ["Z"]
    blobs, pos, lens, raws, infl, base = [], [], [], [], [], 0
    lossy = host.copy() if comp == 5 and ptype == FLOAT else None
    for f in range(n_files):
        blob, p, ln, rw, il = craft(host[f], names, ptype, tile, pool, comp, None if lossy is None else lossy[f])
        blobs.append(blob)
        pos += [base + x for x in p]
        lens += ln
        raws += rw
        infl += il
        base += len(blob)
    if lossy is not None:                                                 # (PXR24 keeps 24 bits of a FLOAT in the chunks that shrink)
        pixels = torch.from_numpy(lossy.reshape(-1)).to(dev)
    del host, lossy
    res = {"files": n_files, "channels": n_ch, "height": H, "width": W, "pixel_type": ptype, "tile": tile, "chunks": len(pos), "pixel_bytes": total,
           "file_bytes": base, "chunks_stored_raw": sum(a == b for a, b in zip(lens, raws)), "compression": comp,
           "trip": int(L.zmi_exr_pxr24_trip()) if comp == 5 else int(L.zmi_exr_trip())}
    b = e.exr_headers(blobs)
    del blobs
    assert all(b.readable) and b.shape(0) == (n_ch, H, W)
    hm, hs = wall(lambda: e.exr_headers(b.data, b.offsets, b.lengths), reps)
    res["headers"] = {"ms_median": round(hm, 4), "ms_spread": round(hs, 4)}
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    _, off, ln, st = e.exr_read(b, out=out, align=4)
    assert bool((st == 0).all()) and int(off[-1]) == total and torch.equal(out, pixels), "the planes are wrong"
    res["read_ms"] = stages(e, lambda: e.exr_read(b, out=out, align=4), reps)
    med, spread = wall(lambda: e.exr_read(b, out=out, align=4), reps)
    res["read"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)}
    res["unzip_share"] = round(res["read_ms"]["unzip"] / med, 4)
    res["unzip_gib_s"] = round(total / res["read_ms"]["unzip"] / 1e-3 / 2 ** 30, 2)
    # the unzip's floor: one read and one write of the same number of bytes
    src = torch.empty_like(out)
    cm, cs = wall(lambda: src.copy_(out), reps)
    res["copy"] = {"ms_median": round(cm, 4), "ms_spread": round(cs, 4), "gib_s": round(total / cm / 1e-3 / 2 ** 30, 2)}
    res["unzip_over_copy"] = round(res["read_ms"]["unzip"] / cm, 3)
    del src
    # the yardstick: the batch decoder on the compressed chunks where they stand, true tables
    keep = [k for k in range(len(pos)) if lens[k] < raws[k]]
    n = len(keep)
    in_off = torch.tensor([pos[k] for k in keep], dtype=torch.int64, device=dev)
    in_len = torch.tensor([lens[k] for k in keep], dtype=torch.int32, device=dev)
    caps = np.array([infl[k] for k in keep], dtype=np.int64)
    cap = torch.from_numpy(caps.astype(np.int32)).to(dev)
    ooff = torch.from_numpy(np.concatenate([[0], np.cumsum(caps)[:-1]])).to(dev)
    olen, ost = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    L.zmi_ctx_set_inflate_out_limit(ctx, total + (1 << 16))

    def yard():
        L.zmi_inflate_batch_dev(ctx, b.data.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, WRAP_ZLIB, out.data_ptr(), ooff.data_ptr(),
                                cap.data_ptr(), olen.data_ptr(), ost.data_ptr(), None)

    med_y, spread_y = wall(yard, reps)
    assert bool((ost == 0).all()) and bool((olen == cap).all())
    L.zmi_ctx_set_inflate_out_limit(ctx, 0)
    res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "gib_s": round(int(caps.sum()) / med_y / 1e-3 / 2 ** 30, 2)}
    res["read_over_yardstick"] = round(med / med_y, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--tiles", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--compression", choices=["zip", "pxr24"], default="zip")
    a = ap.parse_args()
    comp = 5 if a.compression == "pxr24" else 3
    if not torch.cuda.is_available():
        sys.exit("gpu_exr_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "exr_read" if comp == 3 else "exr_read_pxr24", "level": 6, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        if a.frames:
            line["frames_2048x1080_rgba_half"] = measure(e, a.frames, 4, 1080, 2048, HALF, 0, a.reps, pool, comp)
        if a.big:
            line["one_%d_square_rgba_half" % a.big] = measure(e, 1, 4, a.big, a.big, HALF, 0, a.reps, pool, comp)
        if a.tiles:
            across = int(round(a.tiles ** 0.5))
            assert across * across == a.tiles
            line["tiles_256_float"] = measure(e, 1, 1, across * 256, across * 256, FLOAT, 256, a.reps, pool, comp)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
