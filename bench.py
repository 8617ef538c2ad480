#!/usr/bin/env python3
"""bench.py -- GiB/s of raw input compressed at level 6 over 1 MiB synthetic Silesia-like shards (BASELINE.json).

One process per GPU.  torch.distributed / RCCL carries the barrier and the max-over-ranks timing; the compression
itself has no collective (shards are independent streams, round-robin ownership: rank r owns the shards g with
g % world == r, BASELINE.json configs[4]).  A step = one deflate pass over this rank's whole batch of shards, inputs
resident in HBM before the timed region starts.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times --steps steps, writes the
last step's outputs if --dump-outputs DIR is given and prints the headline fields (metric, value, unit, ms_per_step, ratio ...)
and nothing else.  With --full the line also carries what the legs below measure and check:
  roofline       dominant kernel (lz77), algorithmic bytes / live HIP-event time against 8 TB/s
  roundtrip      configs[1]: EVERY compressed shard of the step inflated back on the device and compared with its input
  inflate        configs[2]: 64 Ki gzip members produced by the CPU oracle (the reference's algorithm, not the GPU deflater),
                 inflated in 16 Ki-stream launches, every stream compared with the regenerated plaintext
  levels         configs[3]: level 1 and level 9, GiB/s + ratio + the oracle's ratio at the same level
  pcie_inclusive host buffers in, host buffers out (never `value`)
  stream_abi     configs[0]: one ~15.74 MB stream through deflate() / inflate() of the drop-in library, one thread
  stitch         slab packing over all slots (+ the point-to-point slab exchange at N > 1), outside the timed region, with the memory plan
  real_data      lcet10.txt / paper-100k.pdf / fireworks.jpg tiled to 1 MiB at levels 1 / 6 / 9: gpu, oracle and system-zlib ratios
  cpu_baseline   the oracle's level-6 restatement on the host cores (N = 1 only)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GIB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
SEED = 0x5A4C4942


def usable_cores():
    """host cores this process may actually use: affinity mask capped by the cgroup CPU quota"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, int(q / per + 0.5)))
        except Exception:  # noqa: BLE001
            pass
    return max(1, n)


def _oracle():
    import oracle_lib
    o = oracle_lib.load(rebuild=False)
    o.lib.zo_bench_deflate.restype = C.c_double
    o.lib.zo_bench_deflate.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    o.lib.zo_deflate_shards.restype = C.c_double
    o.lib.zo_deflate_shards.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    return o


def cpu_baseline(shard_bytes, level, budget_s=10.0):
    """oracle level-`level` deflate (C restatement of the reference) of the same synthetic shards on all
    host cores: POSIX threads inside the oracle library (zo_bench_deflate), bounded sample."""
    o = _oracle()
    cores = usable_cores()
    tot = C.c_uint64(0)
    # single thread: 8 shards (one of each class)
    t1 = o.lib.zo_bench_deflate(SEED, 0, 8, shard_bytes, level, 1, C.byref(tot))
    one = 8 * shard_bytes / GIB / t1
    # all cores: size the sample to ~budget_s seconds, a multiple of 8 shards per thread
    per_thread = max(8, int(budget_s / (t1 / 8.0)) // 8 * 8)
    n = min(cores * per_thread, 16384, max(cores * 8, int(24 * GIB / shard_bytes)))
    n -= n % 8
    tall = o.lib.zo_bench_deflate(SEED, 0, n, shard_bytes, level, cores, C.byref(tot))
    # labelled secondary reference: the system's zlib, compress2(level) of the same 8 shards, one thread
    secondary = None
    try:
        import zlib
        shards = [o.gen_shard(i, shard_bytes) for i in range(8)]
        ts = time.perf_counter()
        csz = sum(len(zlib.compress(d, level)) for d in shards)
        tz = time.perf_counter() - ts
        secondary = {"library": "system zlib " + zlib.ZLIB_RUNTIME_VERSION, "single_thread_GiB_s": 8 * shard_bytes / GIB / tz,
                     "ratio": 8 * shard_bytes / float(csz), "sample": "8 x %d B (classes 0-7)" % shard_bytes}
    except Exception:  # noqa: BLE001
        pass
    return {"value": n * shard_bytes / GIB / tall, "unit": "GiB/s", "cores": cores, "kind": "port", "system_zlib": secondary,
            "zlib_rs": zlib_rs_probe(),
            "sample": "%d x %d B synthetic shards (classes 0-7), oracle zo_deflate level %d, %d POSIX threads, %.1f s"
                      % (n, shard_bytes, level, cores, tall),
            "single_thread_GiB_s": one, "ratio": n * shard_bytes / float(tot.value)}


def zlib_rs_probe():
    """SURVEY 8d's first preference for the CPU baseline is zlib-rs itself (libz-rs-sys-cdylib built offline by cargo on the box that
    runs the bench).  That needs a Rust toolchain AND the reference's sources; this records what the box has, so that the question
    is closed with evidence instead of an assumption."""
    import platform
    import shutil
    host = platform.node() or "?"
    try:
        cargo, rustc = shutil.which("cargo"), shutil.which("rustc")
        src = os.environ.get("ZLIB_RS_SRC", "")   # (a checkout of trifectatechfoundation/zlib-rs, if the operator has one on the box)
        if not cargo or not rustc:
            return {"cargo": "absent on %s" % host, "rustc": "absent" if not rustc else rustc, "built": False}
        if not src or not os.path.isfile(os.path.join(src, "libz-rs-sys-cdylib", "Cargo.toml")):
            return {"cargo": cargo, "rustc": rustc, "built": False,
                    "why": "no zlib-rs sources on %s (set ZLIB_RS_SRC to a checkout; the bench never reads /root/reference)" % host}
        import subprocess
        import tempfile
        tgt = tempfile.mkdtemp(prefix="zlib_rs_target_")
        r = subprocess.run([cargo, "build", "--release", "--offline", "--manifest-path", os.path.join(src, "libz-rs-sys-cdylib", "Cargo.toml"),
                            "--target-dir", tgt], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"cargo": cargo, "built": False, "why": r.stderr[-400:]}
        so = [os.path.join(dp, f) for dp, _, fs in os.walk(tgt) for f in fs if f.startswith("libz_rs") and f.endswith(".so")]
        if not so:
            return {"cargo": cargo, "built": False, "why": "no shared library in the target directory"}
        L = C.CDLL(so[0])
        o = _oracle()
        shards = [o.gen_shard(i, 1 << 20) for i in range(8)]
        L.compressBound.restype = C.c_ulong
        L.compressBound.argtypes = [C.c_ulong]
        cap = int(L.compressBound(1 << 20))
        dst = C.create_string_buffer(cap)
        t0 = time.perf_counter()
        csz = 0
        for d in shards:
            dl = C.c_ulong(cap)
            assert L.compress2(dst, C.byref(dl), d, C.c_ulong(len(d)), 6) == 0
            csz += dl.value
        dt = time.perf_counter() - t0
        return {"cargo": cargo, "built": True, "library": so[0], "single_thread_GiB_s": 8 * (1 << 20) / GIB / dt, "ratio": 8 * (1 << 20) / float(csz),
                "sample": "8 x 1 MiB (classes 0-7), compress2(level 6), one thread"}
    except Exception as ex:  # noqa: BLE001
        return {"cargo": "probe failed on %s" % host, "why": repr(ex), "built": False}


def oracle_members(n, shard_bytes, level, wrap, threads):
    """gzip / zlib members of shards 0..n-1 made by the CPU oracle -> (uint8 array [n, stride], lengths, seconds)"""
    import numpy as np
    o = _oracle()
    stride = shard_bytes + shard_bytes // 8 + 4096
    out = np.empty(n * stride, dtype=np.uint8)
    ln = np.zeros(n, dtype=np.uint32)
    dt = o.lib.zo_deflate_shards(SEED, 0, n, shard_bytes, level, wrap, threads, out.ctypes.data, stride, ln.ctypes.data)
    if dt < 0:
        raise RuntimeError("oracle member production failed")
    return out.reshape(n, stride), ln, dt


def csrc_sha16():
    """what the kernels ARE: sha-256 over zlib_rs_amd/csrc/*.hip / *.h (names + contents), first 16 hex digits.  The counter files
    under profiles/ record it (tools/prof_final.sh), and a file collected from other sources is not replayed (the GPU box has no
    .git: a content hash, not a commit)"""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "zlib_rs_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.cpp"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def issue_replay():
    """roofline.issue: what these kernels are actually bound by (instruction issue, not HBM) -- per kernel
    the wave-instructions per byte by class, the SIMD cycles one of them costs and the fraction of VALU lanes that were active,
    from the SQ counter pass of tools/prof_final.sh.  A REPLAYED figure (counters need their own rocprofv3 run): `source` names
    the committed file; the newest profiles/rNN_issue.json wins."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]*_issue.json")))
    if not files:
        return None
    j = json.load(open(files[-1]))
    if j.get("_csrc_sha16") != csrc_sha16():
        return {"stale": "profiles/%s was collected from other kernel sources (%s, now %s): not replayed -- rerun tools/prof_final.sh"
                         % (os.path.basename(files[-1]), j.get("_csrc_sha16", "no hash recorded"), csrc_sha16())}
    nbytes = float(j["bytes_per_launch"])
    out = {"source": "profiles/%s (%s; replayed, not measured in this run)" % (os.path.basename(files[-1]), j.get("_collected", "?")),
           "per": "byte of raw data (deflate kernels: input, inflate kernels: output) of one 16 384 x 1 MiB launch",
           "cycles_per_instr": "SIMD cycles per wave-instruction = SQ_BUSY_CYCLES * 32 / (VALU + SALU + LDS instructions): the chip has 32 "
                               "shader engines counting busy cycles and 1024 SIMDs issuing",
           "lane_util": "SQ_THREAD_CYCLES_VALU / (64 * SQ_INSTS_VALU)", "kernels": {}}
    for name in ("zmi_lz77_kernel_t", "zmi_parse_kernel", "zmi_encode_kernel_t", "zmi_encode_kernel", "zmi_inflate_kernel", "zmi_inflate_resolve_kernel"):
        k = j["kernels"].get(name)
        if not k:
            continue
        tot = k["valu"] + k["salu"] + k["lds"]
        out["kernels"][name] = {"valu_per_byte": round(k["valu"] / nbytes, 3), "salu_per_byte": round(k["salu"] / nbytes, 3),
                                "lds_per_byte": round(k["lds"] / nbytes, 3), "wave_instr_per_byte": round(tot / nbytes, 3),
                                "cycles_per_instr": round(k["busy_cycles"] * 32.0 / tot, 3) if tot else None,
                                "lane_util": round(k["thread_cycles_valu"] / (64.0 * k["valu"]), 3) if k["valu"] else None,
                                "wait_any_frac_of_wave_cycles": round(k["wait_any"] / k["wave_cycles"], 3) if k.get("wave_cycles") else None}
    return out


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start N ranks of this script, one per GPU, with the
    environment torchrun would give them (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT), stdout / stderr
    inherited (rank 0 prints the JSON line).  Returns the first non-zero exit code; a rank that dies takes the others with
    it (they would wait in a barrier forever).  The launcher itself never touches HIP."""
    import socket
    import subprocess
    if n < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    live = set(range(n))
    try:
        while live:
            for r in sorted(live):
                code = procs[r].poll()
                if code is None:
                    continue
                live.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    for q in sorted(live):      # our own children, by their exact PIDs
                        procs[q].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def launch_check(world, rank):
    """--launch-check: the rendezvous of the N ranks and nothing else (backend gloo: runs without a GPU).  The CPU suite uses
    it to see that `--gpus 2` really becomes two ranks (tests/test_bench_launcher.py)."""
    import torch
    import torch.distributed as dist
    if os.environ.get("ZMI_BENCH_FAIL_RANK") == str(rank):   # the test of "a dying rank fails the launch"
        sys.exit(7)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([rank + 1], dtype=torch.int64)
    dist.all_reduce(t)
    assert int(t.item()) == world * (world + 1) // 2
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks_seen": int(t.item()), "backend": "gloo"}))
    dist.barrier()
    dist.destroy_process_group()


def headline(args, world, elapsed, S, B, ratio, checked):
    """the fields every run prints: the timed steps' rate (all ranks' raw bytes / the slowest rank's time) and what was run"""
    return {
        "metric": "GiB/s raw input compressed (level %d, 1 MiB shards)" % args.level,
        "value": S * B * world * args.steps / GIB / elapsed, "unit": "GiB/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed * 1e3 / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": "%d x %d B synthetic Silesia-like shards per GPU, level %d, zlib wrapper; %s" % (S, B, args.level, checked),
                   "shards_per_gpu": S, "shard_bytes": B, "level": args.level,
                   "parallelism": "shard-parallel x%d, round-robin ownership (no data-path collective)" % world},
        "ratio": ratio,
    }


def dump_outputs(d, e, torch, out, olen, st, prefix="", sample=8, budget=48 << 20):
    """--dump-outputs DIR: what the last timed step handed its caller, as float arrays (so that two builds can be compared output
    for output; the inputs are the seeded generator's, the same in every run).  Every shard's compressed length, status and the
    CRC-32 of its compressed stream; the compressed bytes themselves of a fixed, seeded sample of shards (zero past each stream's
    end), as many whole rows of `out` as fit in `budget` bytes of float32."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    S, stride = int(out.shape[0]), int(out.shape[1])
    torch.cuda.synchronize()
    coff = torch.arange(S, dtype=torch.int64, device=out.device) * stride
    _, crc = e.checksums(out.view(-1), coff, olen, adler=False, crc=True)
    torch.cuda.synchronize()
    hl = olen.cpu().numpy().astype(np.int64)
    k = max(1, min(sample, S, budget // (4 * stride)))
    cols = min(stride, budget // (4 * k))
    idx = np.sort(np.random.default_rng(SEED).choice(S, size=k, replace=False))
    rows = out[torch.from_numpy(idx).to(out.device), :cols].cpu().numpy().astype(np.float32)
    rows[np.arange(cols)[None, :] >= hl[idx][:, None]] = 0.0
    arrays = {"out_len": hl.astype(np.float64), "status": st.cpu().numpy().astype(np.float64),
              "compressed_crc32": crc.cpu().numpy().view(np.uint32).astype(np.float64),
              "sample_shards": idx.astype(np.float64), "sample_compressed": rows}
    for name, a in arrays.items():
        np.save(os.path.join(d, prefix + name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shards", type=int, default=int(os.environ.get("ZMI_BENCH_SHARDS", 65536)), help="shards per GPU")
    ap.add_argument("--shard-bytes", type=int, default=1 << 20)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: device round trip of every shard, host check, stitch, roofline, inflate / levels / "
                         "PCIe / stream-ABI / real-data legs and the CPU baseline (the options below that name these legs act only with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--verify", type=int, default=64, help="shards additionally checked on the host with the oracle after timing")
    ap.add_argument("--inflate-members", type=int, default=4096,
                    help="distinct gzip members the CPU oracle produces for the inflate leg (tiled on the device to --shards streams)")
    ap.add_argument("--launch-streams", type=int, default=16384, help="streams per inflate launch (round trip and inflate leg)")
    ap.add_argument("--sweep-shards", type=int, default=16384, help="shards of the level 1 / level 9 sweep (configs[3])")
    ap.add_argument("--pcie-shards", type=int, default=8192, help="shards of the host-buffer (PCIe inclusive) measurement")
    ap.add_argument("--scratch-gib", type=float, default=float(os.environ.get("ZMI_BENCH_SCRATCH_GIB", 70)),
                    help="device scratch of the engine (one launch group of the deflate pipeline): 70 GiB = 16384 shards per launch")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-stitch", action="store_true", help="skip the slab packing / exchange leg")
    ap.add_argument("--stitch-deadline", type=float, default=240.0, help="seconds the multi-GPU slab exchange may take before it is given up")
    ap.add_argument("--no-extras", action="store_true", help="skip the inflate / levels / PCIe legs (profiling runs)")
    ap.add_argument("--stream-abi-only", action="store_true",
                    help="run only the single-stream ABI leg (configs[0]) and print its JSON object: the full run starts this in a process of its own")
    ap.add_argument("--launch-check", action="store_true",
                    help="rendezvous only (gloo, no GPU work): every rank checks world == --gpus, rank 0 prints one JSON line")
    args = ap.parse_args()

    # ---- one process per GPU.  Started under torchrun (the driver's N > 1 form) WORLD_SIZE is set and this process is a
    # rank; started plainly (`python bench.py --gpus N`) this process is the LAUNCHER: it starts N ranks of itself with the
    # torchrun environment and waits for them.  Either way the ranks insist on world == --gpus.
    if "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ["WORLD_SIZE"])
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (python bench.py --gpus N starts them itself)"
                         % (args.gpus, world))
    if args.stream_abi_only:
        print(json.dumps(stream_abi_leg(args.level)))
        return
    if args.launch_check:
        return launch_check(world, rank)

    import numpy as np
    import torch
    import torch.distributed as dist
    from zlib_rs_amd import dist as zdist
    from zlib_rs_amd.engine import Engine, uniform_layout, WRAP_GZIP, WRAP_ZLIB

    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    e = Engine(local, scratch_bytes=int(args.scratch_gib * GIB))
    S, B = args.shards, args.shard_bytes

    # round-robin ownership: local shard j of rank r is global shard j*world + r
    data = e.gen_shards(S, B, first_shard=rank, shard_step=world)
    off, ln = uniform_layout(S, B, dev)
    stride = e.deflate_bound(B, WRAP_ZLIB)
    out = torch.empty((S, stride), dtype=torch.uint8, device=dev)
    olen = torch.empty(S, dtype=torch.int32, device=dev)
    st = torch.empty(S, dtype=torch.int32, device=dev)

    def step():
        e.deflate_batch(data, off, ln, B, level=args.level, wrap=WRAP_ZLIB, out=out, out_len=olen, status=st)

    def timing(on):
        e.L.zmi_ctx_set_timing(e._ctx, 1 if on else 0)

    def take_timing():
        sums, cnts = (C.c_double * 8)(), (C.c_uint32 * 8)()
        e.L.zmi_ctx_get_timing(e._ctx, sums, cnts)
        return list(sums), list(cnts)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    timing(True)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    sums, cnts = take_timing()
    timing(False)
    elapsed = zdist.max_over_ranks(elapsed, dev)

    # ---- correctness outside the timed region ----
    assert int((st != 0).sum().item()) == 0, "deflate reported errors"
    csum = olen.to(torch.int64).sum()
    stitch_obj = None
    if world > 1:
        dist.all_reduce(csum)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, e, torch, out, olen, st, "" if world == 1 else "rank%d_" % rank)
    if not args.full:
        # the plain run: the headline figure and nothing else (every other leg, check and figure is --full)
        if rank == 0:
            print(json.dumps(headline(args, world, elapsed, S, B, S * B * world / int(csum.item()),
                                      "deflate status of every shard checked (the round trips run with --full)")), flush=True)
        if world > 1:
            dist.destroy_process_group()
        e.close()
        return
    if not args.no_stitch and world == 1:
        # (no try / except: a stitch that cannot run is a failed run, not a footnote -- the memory plan says why beforehand)
        plan = memory_plan(torch, world, S, B, stride, args.scratch_gib, float(csum.item()) / GIB + 0.1, 0.0)
        stitch_obj = stitch_leg(e, torch, out, olen, dev)
        stitch_obj["memory_plan"] = plan
        torch.cuda.empty_cache()
    comp_total = int(csum.item())
    raw_total = S * B * world
    ratio = raw_total / comp_total

    # every compressed shard back through the GPU inflater, compared bit-exactly with its input (configs[1])
    LS = max(1, min(S, args.launch_streams))
    back = torch.empty(LS * B, dtype=torch.uint8, device=dev)
    cap = torch.full((LS,), B, dtype=torch.int32, device=dev)
    ooff = torch.arange(LS, dtype=torch.int64, device=dev) * B
    blen = torch.empty(LS, dtype=torch.int32, device=dev)
    bst = torch.empty(LS, dtype=torch.int32, device=dev)
    wcount = min(64, LS)   # first-use costs (scratch allocation, kernel load) stay out of the timing
    e.inflate_batch(out, torch.arange(wcount, dtype=torch.int64, device=dev) * out.stride(0), olen[:wcount].contiguous(), back,
                    ooff[:wcount].contiguous(), cap[:wcount].contiguous(), wrap=WRAP_ZLIB)
    torch.cuda.synchronize()
    rt_s, rt_streams = 0.0, 0
    timing(True)
    for g0 in range(0, S, LS):
        cnt = min(LS, S - g0)
        coff = (torch.arange(cnt, dtype=torch.int64, device=dev) + g0) * out.stride(0)
        torch.cuda.synchronize()
        ti = time.perf_counter()
        e.inflate_batch(out, coff, olen[g0:g0 + cnt].contiguous(), back, ooff[:cnt].contiguous(), cap[:cnt].contiguous(), wrap=WRAP_ZLIB,
                        out_len=blen, status=bst)
        torch.cuda.synchronize()
        rt_s += time.perf_counter() - ti
        assert int((bst[:cnt] != 0).sum().item()) == 0, "inflate of the step's output reported errors"
        assert int((blen[:cnt] != B).sum().item()) == 0
        assert torch.equal(back[:cnt * B], data[g0 * B:(g0 + cnt) * B]), "device round trip failed in shards %d..%d" % (g0, g0 + cnt)
        rt_streams += cnt
    rsums, rcnts = take_timing()
    timing(False)
    roundtrip_obj = {"streams": rt_streams, "of": S, "check": "all streams, bit-exact on device against the input shards",
                     "value": rt_streams * B / GIB / rt_s, "unit": "GiB/s of output", "streams_per_launch": LS,
                     "kernel_ms_per_launch": {"decode": rsums[3] / max(1, rcnts[3]), "resolve": rsums[6] / max(1, rcnts[6]),
                                              "checksum": rsums[0] / max(1, rcnts[0])},
                     "input": "the step's own level-%d zlib streams" % args.level}
    host_checked = 0
    if rank == 0 and args.verify > 0:
        o = _oracle()
        idx = sorted(set([0, S - 1] + list(range(7, S, max(1, S // args.verify)))))[:args.verify + 2]
        hl = olen.cpu().numpy()
        for i in idx:
            comp = bytes(out[i, :int(hl[i])].cpu().numpy())
            rc, bk, _, msg = o.inflate(comp, B, 1)
            assert rc == 1 and bk == o.gen_shard(i * world + rank, B), "round trip failed for shard %d: rc=%d %s" % (i, rc, msg)
        host_checked = len(idx)

    stitch_failed = False
    if not args.no_stitch and world > 1:
        # The stitch across GPUs through the C ABI -- zmi_exchange_sizes, zmi_stitch_plan_dev, zmi_exchange_slabs_round on
        # RCCL -- after everything else of this rank is checked, outside the timed region, under a deadline: this exchange has
        # never run on multi-GPU hardware, and a hung collective must not cost the run its line.
        plan = memory_plan(torch, world, S, B, stride, args.scratch_gib, float(olen.to(torch.int64).sum().item()) / GIB + 0.1,
                           0.5 * (world - 1))
        stitch_obj = with_deadline(lambda: stitch_leg_multi(e, dist, torch, out, olen, dev, world, rank, step=step, step_bytes=S * B,
                                                             step_s=elapsed / args.steps), args.stitch_deadline)
        stitch_obj["memory_plan"] = plan
        stitch_failed = bool(stitch_obj.get("failed"))

    extras = rank == 0 and world == 1 and not args.no_extras
    inflate_obj = levels_obj = pcie_obj = None
    if extras:
        del out
        torch.cuda.empty_cache()
        cores = usable_cores()
        # ---- configs[2]: inflate-only, gzip members made by the CPU oracle ----
        M = max(1, min(args.inflate_members, S))
        members, mlen, prod_s = oracle_members(M, B, 6, 2, cores)
        mstride = members.shape[1]
        d_members = torch.from_numpy(members).to(dev)
        d_mlen = torch.from_numpy(mlen.astype(np.int32)).to(dev)
        comp_bytes = int(mlen.astype(np.int64).sum())
        tiles = max(1, LS // M)
        cntI = tiles * M if LS >= M else LS           # streams per launch: whole tiles of the member set
        sel = torch.arange(cntI, dtype=torch.int64, device=dev) % M
        coffI = sel * mstride
        clenI = d_mlen[sel].contiguous()
        launches = max(1, S // cntI)
        e.inflate_batch(d_members, coffI[:wcount].contiguous(), clenI[:wcount].contiguous(), back, ooff[:wcount].contiguous(),
                        cap[:wcount].contiguous(), wrap=WRAP_GZIP)
        torch.cuda.synchronize()
        inf_s = 0.0
        timing(True)
        for _ in range(launches):
            back.zero_()
            torch.cuda.synchronize()
            ti = time.perf_counter()
            e.inflate_batch(d_members, coffI, clenI, back, ooff[:cntI].contiguous(), cap[:cntI].contiguous(), wrap=WRAP_GZIP, out_len=blen,
                            status=bst)
            torch.cuda.synchronize()
            inf_s += time.perf_counter() - ti
            assert int((bst[:cntI] != 0).sum().item()) == 0 and int((blen[:cntI] != B).sum().item()) == 0
            want = data[:min(M, cntI) * B]
            for t in range(max(1, cntI // M)):
                assert torch.equal(back[t * M * B:t * M * B + want.numel()], want), "inflate of CPU-made members differs"
        isums, icnts = take_timing()
        timing(False)
        nstreams = launches * cntI
        dec_ms, res_ms = isums[3] / max(1, icnts[3]), isums[6] / max(1, icnts[6])
        algo = cntI * B * (1.0 + comp_bytes / float(M * B))   # per launch: 1/ratio B read + 1 B written per output byte
        inflate_obj = {"streams": nstreams, "stream_bytes": B, "streams_per_launch": cntI, "launches": launches,
                       "value": nstreams * B / GIB / inf_s, "unit": "GiB/s of output", "ms_per_launch": inf_s * 1e3 / launches,
                       "kernel_ms_per_launch": {"decode": dec_ms, "resolve": res_ms, "checksum": isums[0] / max(1, icnts[0]),
                                                "verify": isums[4] / max(1, icnts[4])},
                       "roofline_frac": algo / ((dec_ms + res_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS if dec_ms + res_ms > 0 else None,
                       "check": "every stream bit-exact on device against the regenerated plaintext",
                       "input": "%d distinct 1 MiB gzip members produced by the CPU oracle (reference algorithm, level 6, ratio %.3f, "
                                "%d threads, %.1f s), tiled on the device to %d streams per launch"
                                % (M, M * B / float(comp_bytes), cores, prod_s, cntI),
                       "producer_GiB_s": M * B / GIB / prod_s}
        # one launch of 4096 streams (BASELINE configs[2] is quoted on 64 Ki streams; a launch this small is bounded by its
        # slowest stream, one wave each)
        small = min(4096, cntI)
        e.inflate_batch(d_members, coffI[:small].contiguous(), clenI[:small].contiguous(), back, ooff[:small].contiguous(),
                        cap[:small].contiguous(), wrap=WRAP_GZIP, out_len=blen, status=bst)
        torch.cuda.synchronize()
        ti = time.perf_counter()
        e.inflate_batch(d_members, coffI[:small].contiguous(), clenI[:small].contiguous(), back, ooff[:small].contiguous(),
                        cap[:small].contiguous(), wrap=WRAP_GZIP, out_len=blen, status=bst)
        torch.cuda.synchronize()
        small_s = time.perf_counter() - ti
        assert int((bst[:small] != 0).sum().item()) == 0
        for t0_ in range(0, small, M):   # (stream i holds member i % M)
            cnt_ = min(M, small - t0_)
            assert torch.equal(back[t0_ * B:(t0_ + cnt_) * B], data[:cnt_ * B])
        inflate_obj["small_launch"] = {"streams": small, "value": small * B / GIB / small_s, "unit": "GiB/s of output", "ms": small_s * 1e3}
        del d_members
        # ... and members made by the oracle's level 1: the reference's deflate_quick (deflate/algorithm/quick.rs:12-158) emits nothing but
        # FIXED-Huffman blocks (inflate/inffixed_tbl.rs:7), which do not re-synchronise -- the fast pass finds its lanes' starts by
        # walking every bit phase there (inflate.hip inf_fixed_tracks; round 3 decoded such streams 6-8x slower than dynamic ones)
        M1 = max(1, min(2048, M))
        members1, mlen1, prod1_s = oracle_members(M1, B, 1, 2, cores)
        d_m1 = torch.from_numpy(members1).to(dev)
        d_l1 = torch.from_numpy(mlen1.astype(np.int32)).to(dev)
        tiles1 = max(1, LS // M1)
        cnt1 = tiles1 * M1 if LS >= M1 else LS
        sel1 = torch.arange(cnt1, dtype=torch.int64, device=dev) % M1
        coff1 = sel1 * members1.shape[1]
        clen1 = d_l1[sel1].contiguous()
        e.inflate_batch(d_m1, coff1[:wcount].contiguous(), clen1[:wcount].contiguous(), back, ooff[:wcount].contiguous(), cap[:wcount].contiguous(),
                        wrap=WRAP_GZIP)
        torch.cuda.synchronize()
        back.zero_()
        timing(True)
        torch.cuda.synchronize()
        ti = time.perf_counter()
        e.inflate_batch(d_m1, coff1, clen1, back, ooff[:cnt1].contiguous(), cap[:cnt1].contiguous(), wrap=WRAP_GZIP, out_len=blen, status=bst)
        torch.cuda.synchronize()
        f_s = time.perf_counter() - ti
        fsums, fcnts = take_timing()
        timing(False)
        assert int((bst[:cnt1] != 0).sum().item()) == 0 and int((blen[:cnt1] != B).sum().item()) == 0
        for t in range(max(1, cnt1 // M1)):
            assert torch.equal(back[t * M1 * B:(t + 1) * M1 * B], data[:M1 * B]), "inflate of the oracle's level-1 members differs"
        inflate_obj["level1_fixed_blocks"] = {
            "streams": cnt1, "value": cnt1 * B / GIB / f_s, "unit": "GiB/s of output", "ratio": M1 * B / float(mlen1.astype(np.int64).sum()),
            "kernel_ms_per_launch": {"decode": fsums[3] / max(1, fcnts[3]), "resolve": fsums[6] / max(1, fcnts[6])},
            "input": "%d distinct 1 MiB gzip members made by the CPU oracle at level 1 (the reference's deflate_quick: fixed-Huffman blocks only), "
                     "tiled to %d streams, one launch; every stream bit-exact on device" % (M1, cnt1)}
        del d_m1
        # ---- configs[3]: level 1 and level 9 ----
        SW = max(1, min(args.sweep_shards, S))
        out2 = torch.empty((SW, stride), dtype=torch.uint8, device=dev)
        o = _oracle()
        levels_obj = {}
        for lvl in (1, 9):
            wn = min(1024, SW)
            e.deflate_batch(data, off[:wn].contiguous(), ln[:wn].contiguous(), B, level=lvl, wrap=WRAP_ZLIB, out=out2, out_len=olen, status=st)
            torch.cuda.synchronize()
            timing(True)
            ti = time.perf_counter()
            e.deflate_batch(data, off[:SW].contiguous(), ln[:SW].contiguous(), B, level=lvl, wrap=WRAP_ZLIB, out=out2, out_len=olen, status=st)
            torch.cuda.synchronize()
            dt = time.perf_counter() - ti
            lsums, lcnts = take_timing()
            timing(False)
            assert int((st[:SW] != 0).sum().item()) == 0
            csz = int(olen[:SW].to(torch.int64).sum().item())
            # round trip of the sweep output: every stream, on device
            vs = min(SW, LS)
            e.inflate_batch(out2, torch.arange(vs, dtype=torch.int64, device=dev) * out2.stride(0), olen[:vs].contiguous(), back,
                            ooff[:vs].contiguous(), cap[:vs].contiguous(), wrap=WRAP_ZLIB, out_len=blen, status=bst)
            torch.cuda.synchronize()
            assert int((bst[:vs] != 0).sum().item()) == 0 and torch.equal(back[:vs * B], data[:vs * B]), "level %d round trip failed" % lvl
            # the oracle (reference algorithm) at the same level on a sample of the same shards: ratio + rate
            ns = 64 if lvl < 9 else 32
            tot = C.c_uint64(0)
            ts = o.lib.zo_bench_deflate(SEED, 0, ns, B, lvl, min(cores, ns), C.byref(tot))
            gsz = int(olen[:ns].to(torch.int64).sum().item())
            levels_obj["L%d" % lvl] = {"value": SW * B / GIB / dt, "unit": "GiB/s", "ratio": SW * B / float(csz), "shards": SW,
                                       "kernel_ms": {"lz77": lsums[1], "parse": lsums[5], "encode": lsums[2]},
                                       "oracle_ratio_same_shards": ns * B / float(tot.value), "gpu_ratio_same_shards": ns * B / float(gsz),
                                       "oracle_GiB_s": ns * B / GIB / ts, "oracle_sample": "%d shards, %d threads" % (ns, min(cores, ns)),
                                       "check": "%d streams inflated on device, bit-exact" % vs}
        # the levels in between (the reference's own sweep is 0 .. 9, zlib_benchmarks.json blogpost-compress): the same launch size as
        # levels 1 and 9 (until round 5: 1024 shards, not comparable), one timed launch behind a warm-up of 1024 shards, device round
        # trip of the streams; no oracle figures (levels 1 / 6 / 9 have them)
        for lvl in (2, 3, 4, 5, 7, 8):
            wn = SW
            e.deflate_batch(data, off[:min(1024, SW)].contiguous(), ln[:min(1024, SW)].contiguous(), B, level=lvl, wrap=WRAP_ZLIB, out=out2,
                            out_len=olen, status=st)
            torch.cuda.synchronize()
            timing(True)
            ti = time.perf_counter()
            e.deflate_batch(data, off[:wn].contiguous(), ln[:wn].contiguous(), B, level=lvl, wrap=WRAP_ZLIB, out=out2, out_len=olen, status=st)
            torch.cuda.synchronize()
            dt = time.perf_counter() - ti
            lsums, lcnts = take_timing()
            timing(False)
            assert int((st[:wn] != 0).sum().item()) == 0
            csz = int(olen[:wn].to(torch.int64).sum().item())
            vs = min(wn, LS)
            e.inflate_batch(out2, torch.arange(vs, dtype=torch.int64, device=dev) * out2.stride(0), olen[:vs].contiguous(), back,
                            ooff[:vs].contiguous(), cap[:vs].contiguous(), wrap=WRAP_ZLIB, out_len=blen, status=bst)
            torch.cuda.synchronize()
            assert int((bst[:vs] != 0).sum().item()) == 0 and torch.equal(back[:vs * B], data[:vs * B]), "level %d round trip failed" % lvl
            levels_obj["L%d" % lvl] = {"value": wn * B / GIB / dt, "unit": "GiB/s", "ratio": wn * B / float(csz), "shards": wn,
                                       "kernel_ms": {"lz77": lsums[1], "parse": lsums[5], "encode": lsums[2]},
                                       "note": "one launch of %d shards" % wn,
                                       "check": "%d streams inflated on device, bit-exact" % vs}
        del out2
        # ---- PCIe inclusive: host buffers in, host buffers out (zmi_deflate_batch / zmi_inflate_batch, pipelined copies) ----
        # In a process of its own WITHOUT torch (tools/gpu_host_probe.py --json): libzmi355.so binds to whatever HIP runtime the process
        # holds, and inside this process that is the one torch ships (ROCm 7.0), whose copies from and to host memory run 15-30 % below
        # the system's (/opt/rocm, 7.2) -- 29.7 / 24.3 GiB/s here against 35-36 / 34 in a process that is not torch's
        # (gpurun_out/r06z_bench.json, r06_hostprobe2.log).  A caller of the C ABI has the system's runtime.
        P = max(1, min(args.pcie_shards, S))
        if True:   # (a failing host-buffer leg fails the run: VERDICT r03 weak 1)
            child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_host_probe.py"), "--json", "--shards", str(P), "--level", str(args.level),
                                    "--reps", "5"], capture_output=True, text=True, timeout=3000)
            lines = [x for x in child.stdout.splitlines() if x.startswith("{")]
            if child.returncode != 0 or not lines:
                raise RuntimeError("host-buffer leg failed: " + child.stderr[-2000:])
            hp = json.loads(lines[-1])
            pcie_obj = {"value": hp["deflate"]["median"], "unit": "GiB/s", "shards": P, "timing": "median of 5 calls behind a warm-up call", "spread": hp["deflate"],
                        "link": pcie_link_probe(torch, dev),
                        "path": "zmi_deflate_batch: pageable host memory -> pinned staging -> H2D -> kernels -> slab written to pinned host "
                                "memory by the pack kernel -> scattered to the caller's slots; chunks pipelined over three slots",
                        "ratio": hp["ratio"], "inflate_GiB_s": hp["inflate"]["median"], "inflate_spread": hp["inflate"],
                        "inflate_path": "zmi_inflate_batch: pageable host memory -> pinned staging -> H2D -> kernels -> the chunk's output region to "
                                        "pinned host memory -> scattered to the caller's regions; median of 5 calls",
                        "round_trip": hp["round_trip"], "process": hp["process"]}
    del back

    stream_obj = real_obj = None
    if extras:
        # In a process of its own: the single-stream calls of libz_mi355.so measured beside this process's 270 GiB of device tensors and
        # its pinned staging read 1.0 - 1.2 GiB/s for inflate() where a fresh process reads 1.85 - 2.1 (gpurun_out/r06n, r06p): what a
        # caller of the drop-in gets is the latter, and it is what reproduces from run to run.
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--stream-abi-only", "--level", str(args.level)],
                               capture_output=True, text=True, timeout=3000)
        lines = [x for x in child.stdout.splitlines() if x.startswith("{")]
        if child.returncode != 0 or not lines:
            raise RuntimeError("stream ABI leg failed: " + child.stderr[-2000:])
        stream_obj = json.loads(lines[-1])
        stream_obj["process"] = "a process of its own (python bench.py --stream-abi-only)"
        real_obj = real_data_leg(e, torch, dev, B)

    if rank == 0:
        value = raw_total * args.steps / GIB / elapsed
        lz_ms = sums[1] / max(1, cnts[1])
        launches_per_step = max(1, cnts[1] // max(1, args.steps))
        shards_per_launch = S / launches_per_step
        algo_bytes = shards_per_launch * B * (1.0 + 1.0 / ratio)
        achieved = algo_bytes / (lz_ms * 1e-3) / 1e9 if lz_ms > 0 else 0.0
        # measured HBM traffic of the dominant kernel: rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes
        # (tools/prof_final.sh), recorded per launch in profiles/ and scaled to this run's launch size -- a replayed
        # figure, not measured in this run: traffic_source names the file it comes from
        traffic, traffic_source = None, None
        for name in ("r06_traffic.json", "r05_traffic.json"):
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", name)))
                if tj.get("_csrc_sha16") != csrc_sha16():
                    traffic_source = "profiles/%s is stale (collected from kernel sources %s, now %s): not replayed" % (
                        name, tj.get("_csrc_sha16", "without a hash"), csrc_sha16())
                    break
                k = tj.get("zmi_lz77_kernel") or tj.get("zmi_lz77_kernel_t")
                traffic = (k["fetch_bytes_per_launch"] + k["write_bytes_per_launch"]) * shards_per_launch / k["shards_per_launch"]
                traffic_source = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, %s; replayed, scaled to %d shards per launch)" \
                                 % (name, tj.get("_collected", "round 1"), int(shards_per_launch))
                break
            except Exception:  # noqa: BLE001
                continue
        line = headline(args, world, elapsed, S, B, ratio, "all %d compressed shards inflated back on the device and compared "
                                                           "bit-exactly, %d also on the host with the oracle" % (rt_streams, host_checked))
        line.update({
            "roofline": {"bound": "hbm", "kernel": "zmi_lz77_kernel", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "read_only_frac": value * GIB / 1e9 / HBM_PEAK_GBS / max(1, world),
                         # the whole step against the HBM roofline: algorithmic bytes of ALL kernels of a step (1 B read + 1/ratio B
                         # written per input byte) / ms_per_step / 8 TB/s, per GPU
                         "frac_step": S * B * (1.0 + 1.0 / ratio) / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                         "issue": issue_replay(),
                         "kernel_ms": {"checksum": sums[0] / max(1, cnts[0]), "lz77": lz_ms, "parse": sums[5] / max(1, cnts[5]),
                                       "encode": sums[2] / max(1, cnts[2]),
                                       "note": "checksum runs ONCE per step on a side stream beside the first lz77 launch (2.8 ms alone; its events "
                                               "span the time it shares the chip): it is not on the step's critical path; lz77 / parse / encode are "
                                               "per launch group, back to back on the caller's stream"},
                         "launches_per_step": int(launches_per_step)},
            "roundtrip": roundtrip_obj,
        })
        if inflate_obj is not None:
            line["inflate"] = inflate_obj
        if levels_obj is not None:
            levels_obj["L%d" % args.level] = {"value": value, "unit": "GiB/s", "ratio": ratio, "shards": S, "note": "the timed run"}
            line["levels"] = levels_obj
        if pcie_obj is not None:
            line["pcie_inclusive"] = pcie_obj
        if stream_obj is not None:
            line["stream_abi"] = stream_obj
        if real_obj is not None:
            line["real_data"] = real_obj
        attach_stitch(line, stitch_obj)
        if world == 1 and not args.no_cpu:
            cb = cpu_baseline(B, args.level)
            if cb is not None:
                line["cpu_baseline"] = cb
        print(json.dumps(line), flush=True)
    if stitch_failed:
        os._exit(0)   # the communicator may be wedged: no teardown that could hang (the line above says what happened)
    if world > 1:
        dist.destroy_process_group()
    e.close()


def _median_of(fn, runs=5):
    """fn() -> (seconds, result): the median of `runs` timed calls with the spread beside it (a 2 ms single shot is
    noise, and the documentation quoted the top of it) -> (median seconds, {"runs", "min_s", "max_s"}, last result)"""
    ts, res = [], None
    for _ in range(runs):
        dt, res = fn()
        ts.append(dt)
    ts.sort()
    return ts[len(ts) // 2], {"runs": runs, "min_s": ts[0], "max_s": ts[-1]}, res


def _rate(nbytes, med, spread):
    return {"median": nbytes / GIB / med, "min": nbytes / GIB / spread["max_s"], "max": nbytes / GIB / spread["min_s"], "runs": spread["runs"]}


def _inflate_loop(H, lib, comp, wbits, expect_len, chunk=1 << 22):
    """the blogpost-uncompress.rs loop with the output written where it belongs (no Python-side copies inside the timed region):
    input in `chunk` pieces, room in `chunk` pieces; returns (seconds, rc, output bytes object)"""
    strm = H.ZStream()
    assert lib.inflateInit2_(C.byref(strm), wbits, lib.zlibVersion(), C.sizeof(H.ZStream)) == 0
    src = C.create_string_buffer(comp, len(comp))
    dst = C.create_string_buffer(expect_len + chunk)
    pos = got = 0
    rc = 0
    t0 = time.perf_counter()
    while True:
        if strm.avail_in == 0 and pos < len(comp):
            n = min(chunk, len(comp) - pos)
            strm.next_in, strm.avail_in = C.addressof(src) + pos, n
            pos += n
        room = min(chunk, expect_len + chunk - got)
        strm.next_out, strm.avail_out = C.addressof(dst) + got, room
        rc = lib.inflate(C.byref(strm), 0)
        got += room - strm.avail_out
        if rc == 1 or (rc < 0 and rc != -5) or (rc == -5 and strm.avail_in == 0 and pos >= len(comp) and strm.avail_out != 0):
            break
    dt = time.perf_counter() - t0
    unused = strm.avail_in + (len(comp) - pos)
    lib.inflateEnd(C.byref(strm))
    return dt, rc, dst.raw[:got], unused


def _deflate_loop(H, lib, data, level, wbits, chunk=1 << 22):
    """the blogpost-compress.rs loop (input in `chunk` pieces, Z_NO_FLUSH, then Z_FINISH) with the output written where it
    belongs -- no Python-side copies inside the timed region; returns (seconds, compressed bytes)"""
    strm = H.ZStream()
    assert lib.deflateInit2_(C.byref(strm), level, 8, wbits, 8, 0, lib.zlibVersion(), C.sizeof(H.ZStream)) == 0
    src = C.create_string_buffer(data, len(data))
    cap = len(data) + (len(data) >> 3) + 4096
    dst = C.create_string_buffer(cap)
    pos = got = 0
    t0 = time.perf_counter()
    while True:
        n = min(chunk, len(data) - pos)
        strm.next_in, strm.avail_in = C.addressof(src) + pos, n
        pos += n
        flush = 4 if pos >= len(data) else 0   # Z_FINISH / Z_NO_FLUSH
        while True:
            room = min(chunk, cap - got)
            strm.next_out, strm.avail_out = C.addressof(dst) + got, room
            rc = lib.deflate(C.byref(strm), flush)
            assert rc in (0, 1, -5), rc
            got += room - strm.avail_out
            if rc == 1 or (strm.avail_out != 0 and flush != 4) or rc == -5:
                break
        if flush == 4:
            assert rc == 1
            break
    dt = time.perf_counter() - t0
    assert lib.deflateEnd(C.byref(strm)) == 0
    return dt, dst.raw[:got]


def stream_abi_leg(level):
    """BASELINE.json configs[0] (plumbing / reference): one ~15.74 MB input (silesia-small.tar is not in the reference
    checkout: 15 synthetic shards + the bytes that make up the size) through the stream ABI of libz_mi355.so exactly as
    test-libz-rs-sys/examples/blogpost-compress.rs:94-115 drives deflate() -- one stream, input fed in chunks, one thread --
    and back through inflate() (blogpost-uncompress.rs:6-44); beside it the oracle (reference algorithm) on one host thread."""
    import zlib_abi_harness as H
    from zlib_rs_amd import _build
    lib = H.bind(C.CDLL(_build.ABI_LIB))
    o = _oracle()
    total = 15740000
    data = b"".join(o.gen_shard(i, 1 << 20) for i in range(15))
    data += o.gen_shard(15, 1 << 20)[:total - len(data)]
    H.deflate_stream(lib, data[:1 << 20], level=level, wbits=31, chunk_in=1 << 20, chunk_out=1 << 20)   # first-use costs
    def run_deflate():
        dt, comp = _deflate_loop(H, lib, data, level, 31)
        return dt, comp
    td, td_sp, comp = _median_of(run_deflate)
    def run_deflate_one():   # the reference's driver itself: the whole input and Z_FINISH in one deflate() (blogpost-compress.rs:89-113)
        dt, c1 = _deflate_loop(H, lib, data, level, 31, chunk=len(data))
        return dt, c1
    td1, td1_sp, comp1 = _median_of(run_deflate_one)
    assert o.inflate(comp1, len(data), 2)[1] == data
    def run_inflate_own():
        dt, rc, back, unused = _inflate_loop(H, lib, comp, 31, len(data))
        assert rc == 1 and back == data and unused == 0, "stream ABI round trip failed"
        return dt, None
    _inflate_loop(H, lib, comp, 31, len(data))   # (the first pass pays for the staging buffers of this size)
    ti, ti_sp, _ = _median_of(run_inflate_own)
    rc, ocomp = o.deflate(data[:4 << 20], level, 2)
    t0 = time.perf_counter()
    rc, ocomp = o.deflate(data, level, 2)
    to = time.perf_counter() - t0
    assert o.inflate(comp, len(data), 2)[1] == data          # the oracle reads the GPU's stream
    # the same bytes as a stream of the CPU oracle (the reference's algorithm: blocks of 16 383 symbols, no flush points --
    # what an unmodified caller's inflate() meets most often), through inflate() and through one uncompress2()-style call
    def run_inflate_cpu_made():
        dt, rc2, back2, unused2 = _inflate_loop(H, lib, ocomp, 31, len(data))
        assert rc2 == 1 and back2 == data and unused2 == 0, "stream ABI inflate of the oracle's stream failed"
        return dt, None
    _inflate_loop(H, lib, ocomp, 31, len(data))
    ti2, ti2_sp, _ = _median_of(run_inflate_cpu_made)
    import zlib
    zc = zlib.compress(data, level)
    dst = C.create_string_buffer(len(data))
    dl = C.c_ulong(len(data))
    lib.uncompress(dst, C.byref(dl), zc, len(zc))
    def run_uncompress():
        dl = C.c_ulong(len(data))
        t0 = time.perf_counter()
        rc3 = lib.uncompress(dst, C.byref(dl), zc, len(zc))
        dt = time.perf_counter() - t0
        assert rc3 == 0 and dl.value == len(data)
        return dt, None
    tu, tu_sp, _ = _median_of(run_uncompress)
    assert dst.raw[:len(data)] == data
    def run_syszlib():
        t0 = time.perf_counter()
        zlib.decompress(zc)
        return time.perf_counter() - t0, None
    tz, tz_sp, _ = _median_of(run_syszlib, 3)
    small_len = 1 << 20   # (the default mode's 16- and 64-byte pieces: a 1 MiB stream, see chunk_sweep_leg)
    sweep = chunk_sweep_leg(ocomp, len(data), _build.ABI_LIB, small=(o.deflate(data[:small_len], level, 2)[1], small_len))
    return {"input_bytes": len(data), "path": "deflateInit2_(level, gzip) + deflate() in 4 MiB chunks + inflate() back, one thread, host buffers",
            "chunk_sweep": sweep,
            "timing": "every rate of this object is the median of 5 runs (system zlib: 3); the spread of the runs is under `spread`",
            "deflate_GiB_s": len(data) / GIB / td, "deflate_one_call_GiB_s": len(data) / GIB / td1, "ratio_one_call": len(data) / float(len(comp1)),
            "inflate_GiB_s": len(data) / GIB / ti, "ratio": len(data) / float(len(comp)),
            "inflate_of_cpu_made_stream_GiB_s": len(data) / GIB / ti2, "uncompress_of_zlib_stream_GiB_s": len(data) / GIB / tu,
            "system_zlib_inflate_single_thread_GiB_s": len(data) / GIB / tz,
            "spread": {"deflate": _rate(len(data), td, td_sp), "deflate_one_call": _rate(len(data), td1, td1_sp),
                       "inflate": _rate(len(data), ti, ti_sp), "inflate_of_cpu_made_stream": _rate(len(data), ti2, ti2_sp),
                       "uncompress_of_zlib_stream": _rate(len(data), tu, tu_sp), "system_zlib_inflate": _rate(len(data), tz, tz_sp)},
            "oracle_single_thread_GiB_s": len(data) / GIB / to, "oracle_ratio": len(data) / float(len(ocomp)),
            "note": "one stream: deflate = segments of 32 KiB (64 KiB in a call of 8 MiB and more) on the device, encoder pieces of 8 KiB, a launch per 4 MiB chunk handed in; "
                    "inflate of a stream with flush points (this library's own: a marker behind every piece) = the pieces between the markers decoded side by side and stitched (zmi_inflate_split); "
                    "a stream without them (the CPU's) = one workgroup of 16 waves, a pass covers at most one deflate block"}


def chunk_sweep_leg(gz_stream, out_len, abi_lib, small=None):
    """The reference's own inflate benchmark (test-libz-rs-sys/examples/blogpost-uncompress.rs:6-44; zlib_benchmarks.json: input
    chunks 2^4 ... 2^24, the whole output buffer available, Z_NO_FLUSH): one CPU-made gzip stream through inflate() chunk by
    chunk, by tools/chunk_sweep.c (a C loop, compiled here with gcc), once bound to libz_mi355.so and once to the system's zlib."""
    import subprocess
    import tempfile
    chunks = [1 << k for k in range(4, 25, 2)]
    with tempfile.TemporaryDirectory(prefix="zmi_sweep_") as td:
        exe, gz = os.path.join(td, "chunk_sweep"), os.path.join(td, "in.gz")
        subprocess.run(["gcc", "-O2", "-o", exe, os.path.join(ROOT, "tools", "chunk_sweep.c"), "-ldl"], check=True)
        open(gz, "wb").write(gz_stream)
        res = {}
        # eager = the library's default: every inflate() decodes what it was given (a device launch per call: the pieces below
        # 256 bytes are measured on a shorter stream, below); deferred = ZMI_INFLATE_DEFER=1048576 (opt-in, include/zmi355_zlib.h)
        for name, lib, defer, cs in (("system_zlib", "libz.so.1", None, chunks), ("zmi_deferred", abi_lib, "1048576", chunks),
                                     ("zmi_eager", abi_lib, None, [c for c in chunks if c >= 256])):
            env = dict(os.environ)
            env["LD_LIBRARY_PATH"] = os.path.dirname(abi_lib) + ":" + env.get("LD_LIBRARY_PATH", "")
            env.pop("ZMI_INFLATE_DEFER", None)
            if defer:
                env["ZMI_INFLATE_DEFER"] = defer
                env["ZMI_TUNING"] = "1"   # (the override is honoured only with this set)
            r = subprocess.run([exe, lib, gz, str(out_len), "31"] + [str(c) for c in cs], capture_output=True, text=True, env=env, timeout=1800)
            assert r.returncode == 0, r.stderr
            res[name] = {ln.split()[0]: ln.split() for ln in r.stdout.strip().splitlines()}
        # the default mode at 16- and 64-byte pieces: a decode is a device launch whatever it brings (~250 us; profiles/
        # r06_eager_inflate_trace.txt), the 15.7 MB stream would take ten minutes -- measured on a 1 MiB stream of the same data
        # (per byte the same work: the cost is per call), the system zlib on the same stream beside it
        tiny = {}
        if small is not None:
            gz2 = os.path.join(td, "small.gz")
            open(gz2, "wb").write(small[0])
            for name, lib in (("system_zlib", "libz.so.1"), ("zmi_eager", abi_lib)):
                env = dict(os.environ)
                env["LD_LIBRARY_PATH"] = os.path.dirname(abi_lib) + ":" + env.get("LD_LIBRARY_PATH", "")
                env.pop("ZMI_INFLATE_DEFER", None)
                r = subprocess.run([exe, lib, gz2, str(small[1]), "31", "16", "64"], capture_output=True, text=True, env=env, timeout=1800)
                assert r.returncode == 0, r.stderr
                tiny[name] = {ln.split()[0]: ln.split() for ln in r.stdout.strip().splitlines()}
    rows = {}
    for c in chunks:
        b = res["system_zlib"][str(c)]
        row = {"system_zlib_GiB_s": out_len / GIB / float(b[1])}
        for name in ("zmi_deferred", "zmi_eager"):
            a = res[name].get(str(c))
            if a is None:
                continue
            assert int(a[2]) == out_len == int(b[2]) and int(a[3]) == 1 and a[5] == b[5], ("chunk sweep: outputs differ", name, a, b)
            row[name + "_GiB_s"] = out_len / GIB / float(a[1])
            if name == "zmi_deferred":
                row["polls"] = int(a[4])
        if small is not None and str(c) in tiny.get("zmi_eager", {}):
            a, b = tiny["zmi_eager"][str(c)], tiny["system_zlib"][str(c)]
            assert int(a[2]) == small[1] == int(b[2]) and int(a[3]) == 1 and a[5] == b[5], ("chunk sweep (1 MiB stream): outputs differ", a, b)
            row["zmi_eager_GiB_s"] = small[1] / GIB / float(a[1])
            row["zmi_eager_measured_on"] = "a 1 MiB stream (system zlib on it: %.3f GiB/s)" % (small[1] / GIB / float(b[1]))
        rows[str(c)] = row
    return {"chunks": rows, "stream": "the oracle's gzip stream of the same %d bytes (no flush points)" % out_len,
            "modes": "zmi_eager: the default -- every inflate() call decodes what it brought (exact input accounting, the end of the "
                     "stream is found by the call that delivers it); zmi_deferred: ZMI_INFLATE_DEFER=1048576 -- input is taken and "
                     "decoded once 1 MiB has come in (zlib's 'output latency'), `polls` = calls with avail_in = 0 after the last "
                     "piece until Z_STREAM_END",
            "check": "every run: Z_STREAM_END, total_out and the FNV-1a of the output equal the system zlib's"}


def real_data_leg(e, torch, dev, B):
    """the three real fixtures of the reference's test data (lcet10.txt, paper-100k.pdf, fireworks.jpg; xz-packed
    under tests/golden/fixtures), each tiled to one 1 MiB shard, at levels 1 / 6 / 9: ratio of this engine, of the oracle
    (the reference's algorithm) and of the system zlib on the same bytes, with a device round trip of every stream."""
    import lzma
    import zlib
    from zlib_rs_amd.engine import WRAP_ZLIB
    o = _oracle()
    d = os.path.join(ROOT, "tests", "golden", "fixtures")
    names = ("lcet10.txt", "paper-100k.pdf", "fireworks.jpg")
    blobs = []
    for name in names:
        raw = lzma.decompress(open(os.path.join(d, name + ".xz"), "rb").read())
        blobs.append((raw * (B // len(raw) + 1))[:B])
    n = len(blobs)
    data = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).to(dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * B
    ln = torch.full((n,), B, dtype=torch.int32, device=dev)
    back = torch.empty(n * B, dtype=torch.uint8, device=dev)
    cap = torch.full((n,), B, dtype=torch.int32, device=dev)
    res = {"shard_bytes": B, "note": "each fixture tiled to one 1 MiB shard; gpu / oracle (reference algorithm, CPU) / system zlib ratios"}
    for lvl in (1, 6, 9):
        out, olen, st = e.deflate_batch(data, off, ln, B, level=lvl, wrap=WRAP_ZLIB)
        torch.cuda.synchronize()
        assert int((st != 0).sum().item()) == 0
        blen, bst = e.inflate_batch(out, torch.arange(n, dtype=torch.int64, device=dev) * out.stride(0), olen, back, off, cap, wrap=WRAP_ZLIB)
        torch.cuda.synchronize()
        assert int((bst != 0).sum().item()) == 0 and torch.equal(back, data), "real-data round trip failed at level %d" % lvl
        hl = olen.cpu().numpy()
        for i, name in enumerate(names):
            rc, oc = o.deflate(blobs[i], lvl, 1)
            g, orc, z = B / float(hl[i]), B / float(len(oc)), B / float(len(zlib.compress(blobs[i], lvl)))
            res.setdefault(name, {})["L%d" % lvl] = {"gpu": round(g, 4), "oracle": round(orc, 4), "system_zlib": round(z, 4), "gpu_over_oracle": round(g / orc, 4)}
    return res


def pcie_link_probe(torch, dev, nbytes=1 << 30):
    """what the link gives on this box (pinned host memory, one 1 GiB copy each way, and both ways at once): the ceiling of the
    host-buffer legs -- a deflate call moves 1 B in and 1 / ratio B out per input byte"""
    try:
        h1 = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        h2 = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        d1 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d2 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        out = {}
        for what in ("h2d", "d2h", "both"):
            for rep in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if what in ("h2d", "both"):
                    with torch.cuda.stream(s1):
                        d1.copy_(h1, non_blocking=True)
                if what in ("d2h", "both"):
                    with torch.cuda.stream(s2):
                        h2.copy_(d2, non_blocking=True)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            out[what + "_GB_s"] = nbytes / 1e9 / dt
        out["note"] = "pinned memory, 1 GiB per copy; `both`: each direction's rate while the other runs"
        return out
    except Exception as ex:   # (a box without enough pinnable memory: the legs still run)
        return {"failed": repr(ex)}


def memory_plan(torch, world, S, B, stride, scratch_gib, slab_gib, staging_gib):
    """what one rank holds while the stitch runs; fails loudly above 90 % of the device (a silent OOM inside the stitch would
    cost the whole line)"""
    total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory / GIB
    plan = {"input_GiB": S * B / GIB, "slots_GiB": S * stride / GIB, "scratch_GiB": scratch_gib, "slab_GiB": slab_gib,
            "exchange_staging_GiB": staging_gib, "hbm_total_GiB": total}
    plan["sum_GiB"] = plan["input_GiB"] + plan["slots_GiB"] + plan["scratch_GiB"] + plan["slab_GiB"] + plan["exchange_staging_GiB"]
    plan["frac_of_hbm"] = plan["sum_GiB"] / total
    if plan["frac_of_hbm"] > 0.90:
        raise RuntimeError("memory plan of the stitch exceeds 90 %% of the device: %s" % json.dumps(plan))
    return plan


def stitch_leg(e, torch, out, olen, dev):
    """one GPU: the pack kernel over all slots (the exchange has no peer); the slab is checked against the size table and three
    of its members are inflated by Python's zlib"""
    import zlib
    torch.cuda.synchronize()
    e.L.zmi_ctx_set_timing(e._ctx, 1)
    t0 = time.perf_counter()
    slab, so = e.pack_slab(out, olen)
    torch.cuda.synchronize()
    pack_s = time.perf_counter() - t0
    ksums, kcnts = (C.c_double * 8)(), (C.c_uint32 * 8)()
    e.L.zmi_ctx_get_timing(e._ctx, ksums, kcnts)
    e.L.zmi_ctx_set_timing(e._ctx, 0)
    total = int(olen.to(torch.int64).sum().item())
    assert int(so[-1].item()) == total
    hl = olen.cpu().numpy()
    hso = so.cpu().numpy()
    for i in (0, len(hl) // 2, len(hl) - 1):
        member = bytes(slab[int(hso[i]):int(hso[i]) + int(hl[i])].cpu().numpy())
        assert len(zlib.decompress(member)) > 0
    return {"pack_GB_s": total / 1e9 / pack_s, "pack_kernel_GB_s": (total / 1e9 / (ksums[7] * 1e-3)) if ksums[7] > 0 else None,
            "pack_note": "pack_GB_s is wall time incl. the allocation of the slab (28 GiB on a device that is 80 % full); pack_kernel_GB_s the "
                         "scan + copy kernels alone (HIP events)",
            "slab_bytes": total, "slots": int(olen.numel()),
            "exchange": "none (one GPU): zmi_pack_slab_dev over all slots, three members of the slab inflated on the host"}


def attach_stitch(line, stitch_obj):
    """the stitch leg's object into the bench line; N > 1: `value` is the compression alone, value_with_stitch includes the all-gather
    of every slab (tests/test_bench_multi_emu.py drives this, with_deadline and stitch_leg_multi with two ranks on the CPU build)"""
    if stitch_obj is None:
        return line
    line["stitch"] = stitch_obj
    ov = stitch_obj.get("overlap") if isinstance(stitch_obj, dict) else None
    if ov and not ov.get("failed"):
        line["value_with_stitch"] = ov["value_with_stitch"]
    return line


def with_deadline(fn, seconds):
    """run fn() in a thread (the ctypes calls release the GIL) and give up after `seconds`: -> fn's dict, or {"failed": True, ...}"""
    import threading
    box = {}

    def run():
        try:
            box["res"] = fn()
        except Exception as ex:  # noqa: BLE001  (reported in the line; the caller decides what a failure means)
            box["res"] = {"failed": True, "error": repr(ex)[:300]}

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(seconds)
    if th.is_alive():
        return {"failed": True, "error": "the slab exchange did not finish within %.0f s" % seconds}
    return box["res"]


def stitch_leg_multi(e, dist, torch, out, olen, dev, world, rank, chunk_bytes=1 << 29, step=None, step_bytes=0, step_s=None, scatter_out=None):
    """N > 1: size tables -> plan -> slots packed into this rank's slab -> point-to-point slab exchange in rounds of 512 MiB
    with reused staging (8 slabs of ~29 GiB do not fit beside a 64 GiB working set; a real job scatters / writes out round by
    round, here the received chunks are counted and the first round is checked against sums the owners computed).
    All through the C ABI of libzmi355.so (include/zmi355.h); torch.distributed only carries the 128-byte communicator id."""
    torch.cuda.set_device(dev)
    uid = torch.zeros(128, dtype=torch.uint8, device=dev)
    if rank == 0:
        uid = torch.frombuffer(bytearray(e.comm_unique_id()), dtype=torch.uint8).to(dev)
    dist.broadcast(uid, 0)
    comm = e.comm_create(world, rank, bytes(uid.cpu().numpy()))
    S = int(olen.numel())
    table = e.exchange_sizes(comm, olen, world)
    goff, soff, totals = e.stitch_plan(table)
    assert totals[rank] == int(olen.to(torch.int64).sum().item()) and totals[world] == sum(totals[:world])
    assert torch.equal(table[rank], olen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    slab = torch.empty(totals[rank] + 16, dtype=torch.uint8, device=dev)
    e.copy_ranges(out, None, out.stride(0), olen, out.stride(0), slab, soff[rank])
    torch.cuda.synchronize()
    pack_s = time.perf_counter() - t0
    # what every peer must see in round 0 of this rank's slab
    first = min(chunk_bytes, totals[rank])
    mysum = slab[:first].sum(dtype=torch.int64).reshape(1)   # (no int64 copy of half a GiB)
    sums = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(sums, mysum)
    stage = [None if p == rank else torch.empty(min(chunk_bytes, max(16, totals[p])), dtype=torch.uint8, device=dev) for p in range(world)]
    biggest = max(totals[:world])
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got, lo, checked = 0, 0, 0
    while lo < biggest:
        e.exchange_round(comm, slab, totals, lo, chunk_bytes, stage, -1)
        torch.cuda.synchronize()
        for p in range(world):
            if p == rank or lo >= totals[p]:
                continue
            n = min(chunk_bytes, totals[p] - lo)
            got += n
            if lo == 0:
                assert int(stage[p][:n].sum(dtype=torch.int64).item()) == int(sums[p].item()), "slab bytes of rank %d arrived damaged" % p
                checked += 1
        if scatter_out is not None:
            # (small jobs, the tests: every slab fits one round -- the received slabs and this rank's own go to their places in the
            # globally ordered output, the append loop of the reference's recipe, zlib-rs/src/deflate.rs:4145-4221)
            assert lo == 0 and biggest <= chunk_bytes and int(scatter_out.numel()) >= totals[world]
            for p in range(world):
                src = slab if p == rank else stage[p]
                e.copy_ranges(src, soff[p][:S].contiguous(), 0, table[p].contiguous(), out.stride(0), scatter_out, goff[p].contiguous())
            torch.cuda.synchronize()
        lo += chunk_bytes
    torch.cuda.synchronize()
    ex_local = time.perf_counter() - t0
    dist.barrier()
    tmax = torch.tensor([ex_local], dtype=torch.float64, device=dev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    ex_s = float(tmax.item())
    assert got == sum(totals[:world]) - totals[rank]
    # The north star's number -- "shard + all-gather stitch": one more compression step of this rank on its stream WHILE the complete
    # exchange of the previous step's slabs (every slab to every rank, rounds of 512 MiB into the reused staging) runs on a side
    # stream.  value_with_stitch = all ranks' raw bytes / the slower of the two, max over ranks.  (The kernels of a step fill the
    # chip; RCCL's transfers are copies over xGMI with a few workgroups: DESIGN section 5 expects ~0.2 s of exchange under ~1 s of
    # compression.)  value_with_stitch_no_overlap: the step time and the exchange time measured above, added.
    overlap = None
    if step is not None:
      try:   # (its own guard: a failure here must not cost the line the exchange figures measured above)
          side = torch.cuda.Stream(device=dev)
          dist.barrier()
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          step()                                        # enqueued on the current stream, returns at once
          with torch.cuda.stream(side):
              lo = 0
              while lo < biggest:
                  e.exchange_round(comm, slab, totals, lo, chunk_bytes, stage, -1)
                  lo += chunk_bytes
          side.synchronize()
          torch.cuda.synchronize()
          both = time.perf_counter() - t0
          dist.barrier()
          tboth = torch.tensor([both], dtype=torch.float64, device=dev)
          dist.all_reduce(tboth, op=dist.ReduceOp.MAX)
          overlap = {"value_with_stitch": world * step_bytes / GIB / float(tboth.item()), "unit": "GiB/s",
                     "step_and_exchange_s": float(tboth.item()),
                     "value_with_stitch_no_overlap": world * step_bytes / GIB / (step_s + ex_s) if step_s else None,
                     "note": "one compression step on the main stream while every slab of the step before goes to every rank on a side stream"}
      except Exception as ex:  # noqa: BLE001
        overlap = {"failed": True, "error": repr(ex)[:300]}
    e.comm_destroy(comm)
    return {"overlap": overlap, "pack_GB_s": totals[rank] / 1e9 / pack_s, "slab_bytes": totals[rank], "stitched_bytes": totals[world],
            "exchange": "C ABI (zmi_exchange_sizes + zmi_stitch_plan_dev + zmi_exchange_slabs_round on RCCL): all-gather of the slabs by "
                        "grouped ncclSend / ncclRecv, one pair per peer per 512 MiB round, no ring, staging reused; round 0 of every "
                        "peer checked against the owner's byte sum (%d peers)" % checked,
            "exchange_s": ex_s, "received_GB_per_rank": got / 1e9, "exchange_GB_s_per_rank": got / 1e9 / ex_s if ex_s > 0 else None}


if __name__ == "__main__":
    main()
