"""What reading a ZIP archive on the MI355X costs, stage by stage: zmi_zip_directory_dev (locate / walk / parse)
and zmi_zip_inflate_dev (tables and plan / decode / resolve / CRC-32 / verify / stored copies) from the context's event timing, against
the yardstick -- the existing path a caller had before: zmi_inflate_batch_dev_ex with the true tables, then zmi_checksum_batch_dev.

Archives: gen_shards data at level 6, 4096 x 1 MiB entries and 100 000 x 4 KiB entries.  The entries' streams are
zlib.compressobj(6, DEFLATED, -15) -- what zipfile's ZIP_DEFLATED writes -- compressed on a thread pool and framed by the struct.pack
writer below (zipfile itself is one thread: minutes for 4 GiB); zipfile opens every archive and checks a sample of entries.
One JSON line per run; the committed one is profiles/zip_read.json.

    python tools/gpu_zip_probe.py [--big 4096] [--small 100000] [--reps 5] [--out profiles/zip_read.json]
"""
import argparse
import concurrent.futures
import ctypes as C
import io
import json
import os
import struct
import sys
import zipfile
import zlib

os.environ.setdefault("ZMI_TUNING", "1")        # ZMI_ZIP_STAGES below: the directory call's three kernels timed apart
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_RAW   # noqa: E402

SLOTS = {"crc32": 0, "decode": 3, "verify": 4, "plan": 5, "resolve": 6, "stored": 7}


def _deflate(raw):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush()


def build(host, n, size):
    """n entries of `size` bytes -> the archive (ZIP64 end record when it needs one)"""
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        raws = [host[i * size:(i + 1) * size].tobytes() for i in range(n)]
        payloads = list(pool.map(_deflate, raws))
        crcs = list(pool.map(zlib.crc32, raws))
    out, cen = io.BytesIO(), io.BytesIO()
    for i in range(n):
        name = b"shard/%06d.bin" % i
        off = out.tell()
        assert off < 0xFFFFFFFF
        out.write(struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, 8, 0, 0x21, crcs[i], len(payloads[i]), size, len(name), 0) + name)
        out.write(payloads[i])
        cen.write(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 0x0314, 20, 0, 8, 0, 0x21, crcs[i], len(payloads[i]), size, len(name), 0, 0, 0, 0,
                              0o644 << 16, off) + name)
    cd_off, cd = out.tell(), cen.getvalue()
    out.write(cd)
    if n > 0xFFFE or cd_off > 0xFFFFFFFE:
        out.write(struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, len(cd), cd_off))
        out.write(struct.pack("<IIQI", 0x07064B50, 0, cd_off + len(cd), 1))
    out.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(len(cd), 0xFFFFFFFF), min(cd_off, 0xFFFFFFFF), 0))
    blob = out.getvalue()
    zf = zipfile.ZipFile(io.BytesIO(blob))
    infos = zf.infolist()
    assert len(infos) == n
    for i in (0, n // 2, n - 1):
        assert zf.read(infos[i]) == raws[i]
    return blob


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


def measure(e, n, size, reps):
    L, ctx, dev = e.L, e._ctx, e.device
    data = e.gen_shards(n, size)
    torch.cuda.synchronize()
    blob = build(data.cpu().numpy(), n, size)
    z = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    res = {"entries": n, "entry_bytes": size, "archive_bytes": len(blob), "raw_bytes": n * size}
    # the directory, its three kernels apart: ZMI_ZIP_STAGES = k runs the first k
    d = e.zip_directory(z)
    assert d.n_entries == n and bool(d.readable.all())
    res["directory_bytes"] = d.info["cd_size"]
    ent = torch.empty((n, 48), dtype=torch.uint8, device=dev)
    info = torch.zeros(6, dtype=torch.int64, device=dev)
    cum = []
    for stages in (1, 2, 3):
        os.environ["ZMI_ZIP_STAGES"] = str(stages)
        L.zmi_zip_directory_dev(ctx, z.data_ptr(), z.numel(), ent.data_ptr(), n, info.data_ptr(), None)
        torch.cuda.synchronize()
        L.zmi_ctx_set_timing(ctx, 1)
        for _ in range(reps):
            L.zmi_zip_directory_dev(ctx, z.data_ptr(), z.numel(), ent.data_ptr(), n, info.data_ptr(), None)
        sums, cnts = timing(e)
        L.zmi_ctx_set_timing(ctx, 0)
        cum.append(sums[5] / cnts[5])
    del os.environ["ZMI_ZIP_STAGES"]
    res["directory_ms"] = {"locate": round(cum[0], 4), "walk": round(cum[1] - cum[0], 4), "parse": round(cum[2] - cum[1], 4)}
    res["walk_us_per_entry"] = round((cum[1] - cum[0]) * 1e3 / n, 5)
    assert torch.equal(ent, d.entries)
    # the read
    out = torch.empty(n * size, dtype=torch.uint8, device=dev)
    _, off, ln, st = e.zip_read(z, d, out=out)
    assert bool((st == 0).all()) and torch.equal(out, data)
    L.zmi_ctx_set_timing(ctx, 1)
    for _ in range(reps):
        e.zip_read(z, d, out=out)
    sums, cnts = timing(e)
    L.zmi_ctx_set_timing(ctx, 0)
    res["read_ms"] = {k: round(sums[s] / reps, 4) for k, s in SLOTS.items()}
    med, spread = wall(lambda: e.zip_read(z, d, out=out), reps)
    res["read"] = {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(n * size / med / 1e-3 / 2 ** 30, 2)}
    total_dir = cum[2]
    res["directory_share_of_open_and_read"] = round(total_dir / (total_dir + med), 4)
    # the yardstick: the batch decoder with the true tables, then the checksum call
    host = d.entries.cpu().numpy()
    in_off = torch.from_numpy(host[:, 0:8].copy().view("<i8")[:, 0].copy()).to(dev)
    in_len = torch.from_numpy(host[:, 16:20].copy().view("<i4")[:, 0].copy()).to(dev)
    cap = torch.full((n,), size, dtype=torch.int32, device=dev)
    ooff = torch.arange(n, dtype=torch.int64, device=dev) * size
    olen, ost = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    used, det = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    crc = torch.zeros(n, dtype=torch.int32, device=dev)
    L.zmi_ctx_set_inflate_out_limit(ctx, n * size + (1 << 16))
    out.zero_()

    def yard():
        L.zmi_inflate_batch_dev_ex(ctx, z.data_ptr(), in_off.data_ptr(), in_len.data_ptr(), n, WRAP_RAW, out.data_ptr(), ooff.data_ptr(),
                                   cap.data_ptr(), olen.data_ptr(), ost.data_ptr(), used.data_ptr(), det.data_ptr(), None)
        L.zmi_checksum_batch_dev(ctx, out.data_ptr(), ooff.data_ptr(), olen.data_ptr(), n, 2, None, crc.data_ptr(), None)

    med_y, spread_y = wall(yard, reps)
    assert bool((ost == 0).all()) and torch.equal(out, data) and torch.equal(crc, d.crc32)
    L.zmi_ctx_set_inflate_out_limit(ctx, 0)
    res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "gib_s": round(n * size / med_y / 1e-3 / 2 ** 30, 2)}
    res["read_over_yardstick"] = round(med / med_y, 4)
    res["open_and_read_over_yardstick"] = round((total_dir + med) / med_y, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--small", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_zip_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, u64, i32 = e.L, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    L.zmi_inflate_batch_dev_ex.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    line = {"probe": "zip_read", "level": 6, "reps": a.reps, "device": torch.cuda.get_device_name(0), "walk_tile": int(L.zmi_zip_walk_tile()),
            "big": measure(e, a.big, 1 << 20, a.reps), "small": measure(e, a.small, 4096, a.reps)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
