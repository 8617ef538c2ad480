"""What writing OpenEXR files with ZIP compression on the MI355X costs, stage by stage: zmi_exr_write_dev (tables,
places, pack and raw gather / forward zip / Adler-32 / match search, parse, encode / fixed bytes and words) from the context's event
timing, against two yardsticks: the whole call against the nearest thing a caller had, zmi_deflate_batch_dev(ZMI_WRAP_ZLIB) on the same,
already zipped chunks with hand-made tables -- the transform and the framing left out, in the yardstick's favour; the forward kernel's
event slot against a plain device copy of the same bytes read plus written, its memory floor, the two taking turns inside every repeat.

Pixels: gen_shards data, the planes of the regions as they stand.  Workloads, those of tools/gpu_exr_probe.py: 64 frames of 2048 x 1080
RGBA HALF in chunks of 16 scanlines; one 4096 x 4096 RGBA HALF; 4096 tiles of 256 x 256 FLOAT in one file.  Every written batch is read
back by zmi_exr_read_dev and compared with the pixels.  One JSON line per run; the committed one is profiles/exr_write.json.

--compression pxr24 writes the same workloads with compression 5: the PXR24 forward kernel in the forward slot,
the yardstick on the chunks' forward bytes (m a chunk, made on the host), and FLOAT pixels read back as f24(..) << 8 in the chunks that
were not stored raw.  The committed line is in profiles/exr_pxr24.json.

    python tools/gpu_exr_write_probe.py [--compression zip] [--frames 64] [--big 4096] [--tiles 4096] [--reps 5] [--out profiles/exr_write.json]
"""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_ZLIB   # noqa: E402
from gpu_exr_probe import HALF, FLOAT, f24, pxr24_forward   # noqa: E402  (tools/: the host side of PXR24)

SLOTS = {"adler": 0, "match": 1, "encode": 2, "forward": 3, "words": 4, "parse": 5, "tables_pack_gather": 7}


def zip_forward(raw):
    """raw bytes of a chunk (uint8 array) -> the bytes a ZIP writer hands to zlib"""
    t = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int16)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 0xFF
    return d.astype(np.uint8)


def timing(e):
    sums, cnts = (C.c_double * 8)(), (C.c_uint32 * 8)()
    e.L.zmi_ctx_get_timing(e._ctx, sums, cnts)
    return list(sums)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[-1] - xs[0]


def measure(e, n_files, n_ch, H, W, dtype, tile, reps, pool, compression="zip"):
    dev = e.device
    size = 2 if dtype == torch.float16 else 4
    total = n_files * n_ch * H * W * size
    pixels = e.gen_shards((total + (1 << 20) - 1) >> 20, 1 << 20)[:total].contiguous()
    # HALF bit patterns of gen_shards data include NaNs, which are pixels like any other to a lossless writer; the tensor is only viewed
    images = pixels.view(dtype).view(n_files, n_ch, H, W)
    names = ["A", "B", "G", "R"][:n_ch] if n_ch > 1 else ["Z"]
    kw = dict(channels=names, tile=tile or None, level=6, piece_bytes=1 << 20, align=16)
    if compression != "zip":
        kw["compression"] = compression
    bound = e.exr_bound((H, W), [(n, dtype) for n in names], n_files, tile=tile or None)
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    _, off, ln, st = e.exr_write(images, out=out, **kw)
    assert bool((st == 0).all())
    off_h, ln_h = off.tolist(), ln.tolist()
    clen = e.last_exr_chunk_len.cpu().numpy()
    # read back through the library's reader
    b = e.exr_headers(out, off[:-1].contiguous(), ln)
    assert all(b.readable) and b.shape(0) == (n_ch, H, W)
    back = torch.empty(total, dtype=torch.uint8, device=dev)
    _, _, _, rst = e.exr_read(b, out=back, align=4)
    th, tw = (tile, tile) if tile else (16, W)
    boxes = [(x0, y0, min(tw, W - x0), min(th, H - y0)) for y0 in range(0, H, th) for x0 in range(0, W, tw)]
    raws = [w * h * n_ch * size for _, _, w, h in boxes] * n_files
    want = pixels
    if compression == "pxr24" and dtype == torch.float32:
        # PXR24 keeps 24 bits of a FLOAT in the chunks that shrank (one file of one channel in whole tiles: the mask is a grid)
        assert n_files == 1 and n_ch == 1 and tile and H % tile == 0 and W % tile == 0
        bits = pixels.cpu().numpy().view("<u4").reshape(H, W)
        shrank = (clen.reshape(H // tile, W // tile) != tile * tile * size).repeat(tile, axis=0).repeat(tile, axis=1)
        want = torch.from_numpy(np.where(shrank, f24(bits) << np.uint32(8), bits).astype("<u4").view(np.uint8).reshape(-1)).to(dev)
    assert bool((rst == 0).all()) and torch.equal(back, want), "the written files do not read back as the pixels"
    del back, b, want
    res = {"files": n_files, "channels": n_ch, "height": H, "width": W, "pixel_bytes_each": size, "tile": tile, "chunks": len(raws),
           "pixel_bytes": total, "file_bytes": int(sum(ln_h)), "chunks_stored_raw": int((clen.reshape(-1) == np.array(raws)).sum()),
           "compression": compression, "trip": int(e.L.zmi_exr_pxr24_trip()) if compression == "pxr24" else int(e.L.zmi_exr_zip_trip())}

    def call():
        e.exr_write(images, out=out, **kw)

    # the whole call, and per repeat the forward kernel's slot and a device copy of as many bytes, in turns
    src, dst = torch.empty(total, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    call()
    dst.copy_(src)
    torch.cuda.synchronize()
    walls, fwd, copies, slots = [], [], [], {k: 0.0 for k in SLOTS}
    for _ in range(reps):
        walls.append(event_ms(call))
        e.L.zmi_ctx_set_timing(e._ctx, 1)
        call()
        sums = timing(e)
        e.L.zmi_ctx_set_timing(e._ctx, 0)
        fwd.append(sums[SLOTS["forward"]])
        for k, s in SLOTS.items():
            slots[k] += sums[s] / reps
        copies.append(event_ms(lambda: dst.copy_(src)))
    del src, dst
    m, s = med(walls)
    res["write"] = {"ms_median": round(m, 3), "ms_spread": round(s, 3), "gib_s": round(total / m / 1e-3 / 2 ** 30, 2)}
    res["write_ms"] = {k: round(v, 4) for k, v in slots.items()}
    fm, fs = med(fwd)
    cm, cs = med(copies)
    res["forward"] = {"ms_median": round(fm, 4), "ms_spread": round(fs, 4), "gib_s": round(total / fm / 1e-3 / 2 ** 30, 2)}
    res["copy"] = {"ms_median": round(cm, 4), "ms_spread": round(cs, 4), "gib_s": round(total / cm / 1e-3 / 2 ** 30, 2)}
    res["forward_over_copy"] = round(fm / cm, 3)
    res["encoder_share"] = round((slots["match"] + slots["parse"] + slots["encode"]) / sum(slots.values()), 4)

    # the yardstick: the batch encoder on the zipped chunks, made on the host, every chunk at a multiple of 16
    host = pixels.cpu().numpy().reshape(n_files, n_ch, H, W * size)

    def one(job):
        f, (x0, y0, w, h) = job
        rows = np.ascontiguousarray(host[f, :, y0:y0 + h, x0 * size:(x0 + w) * size].transpose(1, 0, 2))
        if compression == "pxr24":
            return np.frombuffer(pxr24_forward(rows, HALF if size == 2 else FLOAT)[0], dtype=np.uint8)
        return zip_forward(rows.reshape(-1))

    ds = list(pool.map(one, [(f, box) for f in range(n_files) for box in boxes]))
    offs = np.zeros(len(ds), dtype=np.int64)
    at = 0
    for k, d in enumerate(ds):
        offs[k] = at
        at += (d.size + 15) & ~15
    flat = np.zeros(at + 64, dtype=np.uint8)
    for k, d in enumerate(ds):
        flat[offs[k]:offs[k] + d.size] = d
    del host
    d_in, d_off = torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev)
    d_len = torch.tensor([d.size for d in ds], dtype=torch.int32, device=dev)
    max_len = max(d.size for d in ds)
    del ds
    yo, yl, ys = e.deflate_batch(d_in, d_off, d_len, max_len, level=6, wrap=WRAP_ZLIB)
    torch.cuda.synchronize()
    assert bool((ys == 0).all())

    def yard():
        e.deflate_batch(d_in, d_off, d_len, max_len, level=6, wrap=WRAP_ZLIB, out=yo, out_len=yl, status=ys)

    yard()
    torch.cuda.synchronize()
    ym, ysp = med([event_ms(yard) for _ in range(reps)])
    res["yardstick"] = {"ms_median": round(ym, 3), "ms_spread": round(ysp, 3), "gib_s": round(total / ym / 1e-3 / 2 ** 30, 2),
                        "stream_bytes": int(yl.sum().item())}
    res["write_over_yardstick"] = round(m / ym, 4)
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
    comp = a.compression
    if not torch.cuda.is_available():
        sys.exit("gpu_exr_write_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    line = {"probe": "exr_write" if comp == "zip" else "exr_write_pxr24", "level": 6, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        if a.frames:
            line["frames_2048x1080_rgba_half"] = measure(e, a.frames, 4, 1080, 2048, torch.float16, 0, a.reps, pool, comp)
        if a.big:
            line["one_%d_square_rgba_half" % a.big] = measure(e, 1, 4, a.big, a.big, torch.float16, 0, a.reps, pool, comp)
        if a.tiles:
            across = int(round(a.tiles ** 0.5))
            assert across * across == a.tiles
            line["tiles_256_float"] = measure(e, 1, 1, across * 256, across * 256, torch.float32, 256, a.reps, pool, comp)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
