"""What writing a ZIP archive on the MI355X costs: zmi_zip_write_dev between device events and by the
context's event-timing slots, against the yardstick -- what a caller had before it, with the host framing left out in the yardstick's
favour: zmi_deflate_batch_dev(raw) + zmi_checksum_batch_dev + zmi_pack_slab_dev on the same shards.

gen_shards data at level 6 and at level 0, three cases: 100 000 x 4 KiB entries (piece_bytes 4096, and once more with the default of
1 MiB), 4096 x 1 MiB entries, and one 1 GiB entry beside 10 000 x 4 KiB -- which the batch encoder cannot take as one batch under the
default scratch limit, so it has no yardstick.  Every archive is opened once by zipfile (count, a sample of entries read) and by
Engine.zip_read (every entry; in the skewed case every entry but the 1 GiB one, which the batch decoder would read on one workgroup).
One JSON line per run; the committed one is profiles/zip_write.json.

    python tools/gpu_zip_write_probe.py [--small 100000] [--big 4096] [--skew-mib 1024] [--skew-small 10000] [--reps 5] [--out FILE]

Kernel by kernel (profiles/zip_write_kernel_trace.txt): --trace CASE:LEVEL makes exactly three zmi_zip_write_dev calls of one case
(small, small_piece_1mib, big, skewed) and nothing else, for a kernel trace of its own process; a kernel's total over three is its
time per call.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_zip_write_probe.py --trace small:6
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import zipfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch            # noqa: E402
from zlib_rs_amd.engine import Engine, WRAP_RAW   # noqa: E402

SLOTS = {"crc32": 0, "lz77": 1, "parse": 5, "encode": 2, "framing": 7}


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


def opened(e, z, d, data, off, ln, skip_first):
    """zipfile: the count and three entries; Engine.zip_read: every entry (but the first where it is the 1 GiB one)"""
    n = int(ln.numel())
    host_off, host_len = off.tolist(), ln.tolist()
    with zipfile.ZipFile(io.BytesIO(z.cpu().numpy().tobytes())) as zf:
        infos = zf.infolist()
        assert len(infos) == n
        for i in (0, n // 2, n - 1):
            assert zf.read(infos[i]) == data[host_off[i]:host_off[i] + host_len[i]].cpu().numpy().tobytes(), i
    first = 1 if skip_first else 0
    sel = torch.arange(first, n, dtype=torch.int32, device=e.device)
    out, ooff, olen, st = e.zip_read(z, d, indices=sel)
    assert not bool(st.any()) and torch.equal(out, data[host_off[first]:])


def measure(e, data, off, ln, max_len, piece_bytes, level, reps, yardstick, skip_first=False):
    L, ctx, dev = e.L, e._ctx, e.device
    n, total = int(ln.numel()), int(data.numel())
    names = ["shard/%06d.bin" % i for i in range(n)]
    blob, noff, names_bytes = e._zip_names(names)
    out = torch.empty(e.zip_bound(n, names_bytes, total, piece_bytes, level), dtype=torch.uint8, device=dev)
    z, d = e.zip_write(data, off, ln, (blob, noff), level=level, piece_bytes=piece_bytes, directory=True, out=out)
    size = int(z.numel())
    opened(e, z, d, data, off, ln, skip_first)
    del z, d
    meta = torch.zeros(2, dtype=torch.int64, device=dev)

    def write():
        L.zmi_zip_write_dev(ctx, data.data_ptr(), off.data_ptr(), ln.data_ptr(), n, total, blob.data_ptr(), noff.data_ptr(), None, None,
                            piece_bytes, level, 0, 0, out.data_ptr(), out.numel(), meta.data_ptr(), None, None, meta.data_ptr() + 8, None)

    med, spread = wall(write, reps)
    assert meta.tolist() == [size, 0]
    L.zmi_ctx_set_timing(ctx, 1)
    for _ in range(reps):
        write()
    sums, _ = timing(e)
    L.zmi_ctx_set_timing(ctx, 0)
    res = {"entries": n, "raw_bytes": total, "piece_bytes": piece_bytes, "archive_bytes": size, "ratio": round(total / size, 4),
           "write": {"ms_median": round(med, 3), "ms_spread": round(spread, 3), "gib_s": round(total / med / 1e-3 / 2 ** 30, 2)},
           "slot_ms": {k: round(sums[s] / reps, 4) for k, s in SLOTS.items()}}
    res["framing_share"] = round(res["slot_ms"]["framing"] / sum(res["slot_ms"].values()), 4)
    if yardstick:
        stride = e.deflate_bound(max_len, WRAP_RAW)
        slots = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        slab = torch.empty(n * stride, dtype=torch.uint8, device=dev)
        olen, st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        crc, soff = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)

        def yard():
            if level:
                L.zmi_deflate_batch_dev(ctx, data.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, level, 0, WRAP_RAW, slots.data_ptr(),
                                        stride, olen.data_ptr(), st.data_ptr(), None)
            L.zmi_checksum_batch_dev(ctx, data.data_ptr(), off.data_ptr(), ln.data_ptr(), n, 2, None, crc.data_ptr(), None)
            if level:
                L.zmi_pack_slab_dev(ctx, slots.data_ptr(), stride, olen.data_ptr(), n, slab.data_ptr(), slab.numel(), soff.data_ptr(), None)
            else:           # stored: the entries copied densely
                L.zmi_scan_sizes_dev(ctx, ln.data_ptr(), n, soff.data_ptr(), None)
                L.zmi_copy_ranges_dev(ctx, data.data_ptr(), off.data_ptr(), 0, ln.data_ptr(), n, max_len, slab.data_ptr(), soff.data_ptr(),
                                      slab.numel(), None)

        med_y, spread_y = wall(yard, reps)
        assert not bool(st.any())
        res["yardstick"] = {"ms_median": round(med_y, 3), "ms_spread": round(spread_y, 3), "slab_bytes": int(soff[n].item())}
        res["write_over_yardstick"] = round(med / med_y, 4)
    return res


def uniform(e, n, size):
    data = e.gen_shards(n, size)
    return data, torch.arange(n, dtype=torch.int64, device=e.device) * size, torch.full((n,), size, dtype=torch.int32, device=e.device)


def skewed(e, big_mib, n_small):
    """one entry of big_mib MiB, then n_small of 4 KiB"""
    data = torch.cat([e.gen_shards(big_mib, 1 << 20), e.gen_shards(n_small, 4096, first_shard=big_mib)])
    big = big_mib << 20
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=e.device), big + torch.arange(n_small, dtype=torch.int64, device=e.device) * 4096])
    ln = torch.cat([torch.tensor([big], dtype=torch.int32, device=e.device), torch.full((n_small,), 4096, dtype=torch.int32, device=e.device)])
    return data, off, ln


def case_data(e, a, case):
    """-> data, offsets, lengths, piece_bytes of one of the probe's cases"""
    if case in ("small", "small_piece_1mib"):
        return uniform(e, a.small, 4096) + (4096 if case == "small" else 1 << 20,)
    if case == "big":
        return uniform(e, a.big, 1 << 20) + (1 << 20,)
    if case == "skewed":
        return skewed(e, a.skew_mib, a.skew_small) + (1 << 20,)
    sys.exit("--trace: no case %r" % case)


def trace(e, a):
    """three calls of one case and a check of their status: what a kernel trace of this process then holds"""
    case, _, level = a.trace.partition(":")
    level = int(level or 6)
    data, off, ln, piece_bytes = case_data(e, a, case)
    n, total = int(ln.numel()), int(data.numel())
    blob, noff, names_bytes = e._zip_names(["shard/%06d.bin" % i for i in range(n)])
    out = torch.empty(e.zip_bound(n, names_bytes, total, piece_bytes, level), dtype=torch.uint8, device=e.device)
    meta = torch.zeros(2, dtype=torch.int64, device=e.device)
    for _ in range(3):
        rc = e.L.zmi_zip_write_dev(e._ctx, data.data_ptr(), off.data_ptr(), ln.data_ptr(), n, total, blob.data_ptr(), noff.data_ptr(), None,
                                   None, piece_bytes, level, 0, 0, out.data_ptr(), out.numel(), meta.data_ptr(), None, None,
                                   meta.data_ptr() + 8, None)
        assert rc == 0, rc
    size, status = meta.tolist()
    assert status == 0, status
    print(json.dumps({"probe": "zip_write_trace", "case": case, "level": level, "calls": 3, "archive_bytes": size}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=100000)
    ap.add_argument("--big", type=int, default=4096)
    ap.add_argument("--skew-mib", type=int, default=1024)
    ap.add_argument("--skew-small", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, metavar="CASE:LEVEL")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_zip_write_probe needs an MI355X: nothing is measured without one")
    e = Engine(0)
    L, vp, u32, i32 = e.L, C.c_void_p, C.c_uint32, C.c_int
    L.zmi_ctx_set_timing.argtypes = [vp, i32]
    L.zmi_ctx_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u32)]
    if a.trace:
        trace(e, a)
        e.close()
        return
    line = {"probe": "zip_write", "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for level in (6, 0):
        key = "level%d" % level
        line[key] = {}
        data, off, ln = uniform(e, a.small, 4096)
        line[key]["small"] = measure(e, data, off, ln, 4096, 4096, level, a.reps, True)
        if level:
            line[key]["small_piece_1mib"] = measure(e, data, off, ln, 4096, 1 << 20, level, a.reps, False)
        data, off, ln = uniform(e, a.big, 1 << 20)
        line[key]["big"] = measure(e, data, off, ln, 1 << 20, 1 << 20, level, a.reps, True)
        data, off, ln = skewed(e, a.skew_mib, a.skew_small)
        line[key]["skewed"] = measure(e, data, off, ln, 1 << 20, 1 << 20, level, a.reps, False, skip_first=True)
        del data, off, ln
        print(key, json.dumps(line[key]), flush=True)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
