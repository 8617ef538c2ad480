"""CPU tests of the single-stream (pigz-style) deflate on the device: zmi_deflate_stream_dev, zmi_deflate_pieces_dev,
zmi_checksum_combine_dev and zmi_stream_frame_dev (include/zmi355.h; csrc/checksum.hip, pack.hip, zmi_api.hip) on the emulator
build.  The contract is the reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221 (split_deflate): ONE stream,
every piece but the last behind a flush marker, the wrapper once, the trailer from the combined check values.  What is checked:
the stream reads back as one stream (zlib.decompressobj reaches eof with nothing left over), the header equals this library's
deflate(), the piece index marks restart points, the device combine equals the system zlib's crc32_combine64 / adler32_combine64,
the bytes do not depend on the scratch limit or the launch grouping, and the multi-rank form (separate processes against
tests/emu/libmock_rccl.so) is byte-identical to one independent-mode call."""
import ctypes as C
import multiprocessing as mp
import os
import random
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libzmi355_emu.so")
WBITS = {0: -15, 1: 15, 2: 31}
INDEPENDENT = 1
MARKER = b"\x00\x00\xff\xff"


def _p(a):
    return a.ctypes.data


def _bind(L):
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_ctx_create.argtypes = [C.POINTER(vp), i32]
    L.zmi_ctx_destroy.argtypes = [vp]
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    L.zmi_deflate_stream_bound.restype = u64
    L.zmi_deflate_stream_bound.argtypes = [u64, u32, i32]
    L.zmi_stream_header_bytes.restype = u32
    L.zmi_stream_header_bytes.argtypes = [i32]
    L.zmi_deflate_pieces_stride.restype = u64
    L.zmi_deflate_pieces_stride.argtypes = [u32]
    L.zmi_deflate_stream_dev.argtypes = [vp, vp, u64, u32, i32, i32, i32, u32, vp, u64, vp, vp, vp, vp]
    L.zmi_deflate_pieces_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, u32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_checksum_combine_dev.argtypes = [vp, i32, vp, vp, u32, u32, vp, vp, vp]
    L.zmi_stream_frame_dev.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, u64, vp, vp, vp]
    L.zmi_pack_slab_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp]
    L.zmi_copy_ranges_dev.argtypes = [vp, vp, vp, u64, vp, u32, u32, vp, vp, u64, vp]
    L.zmi_comm_unique_id.argtypes = [vp]
    L.zmi_comm_create.argtypes = [C.POINTER(vp), vp, i32, i32, vp]
    L.zmi_comm_destroy.argtypes = [vp]
    L.zmi_exchange_sizes.argtypes = [vp, vp, u32, vp, vp]
    L.zmi_stitch_plan_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.zmi_exchange_slabs.argtypes = [vp, vp, vp, vp, u64, i32, vp]
    return L


def _load(rebuild=True):
    if rebuild:
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")], check=True)
    return _bind(C.CDLL(EMU))


class _Ctx:
    def __init__(self, L):
        self.L = L
        self.ctx = C.c_void_p()
        assert L.zmi_ctx_create(C.byref(self.ctx), 0) == 0

    def close(self):
        self.L.zmi_ctx_destroy(self.ctx)

    def ok(self, rc, what):
        assert rc == 0, "%s: %d %s" % (what, rc, self.L.zmi_last_error().decode())

    def stream(self, data, piece, wrap, flags=0, level=6, strategy=0):
        """one zmi_deflate_stream_dev call -> (stream bytes, piece index)"""
        L, n = self.L, len(data)
        inp = np.frombuffer(bytes(data) + b"\0" * 16, dtype=np.uint8).copy()
        cap = int(L.zmi_deflate_stream_bound(n, piece, wrap))
        out = np.full(cap + 64, 0xA5, dtype=np.uint8)
        olen = np.zeros(1, dtype=np.uint64)
        st = np.full(1, 77, dtype=np.int32)
        npc = max(1, -(-n // piece))
        idx = np.zeros(npc + 1, dtype=np.uint64)
        self.ok(L.zmi_deflate_stream_dev(self.ctx, _p(inp), n, piece, level, strategy, wrap, flags, _p(out), cap, _p(olen), _p(idx),
                                         _p(st), None), "zmi_deflate_stream_dev")
        assert int(st[0]) == 0 and int(olen[0]) <= cap
        assert (out[int(olen[0]):] == 0xA5).all()          # nothing written behind the stream
        return bytes(out[:int(olen[0])]), [int(x) for x in idx]


def _data(n, seed):
    """compressible text-like bytes with some repeats (what a flush boundary must carry history across)"""
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
        if rnd.random() < 0.01:
            out += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 40)))
    return bytes(out[:n])


def _one_stream(s, wrap, want):
    d = zlib.decompressobj(WBITS[wrap])
    got = d.decompress(s)
    assert d.eof and d.unused_data == b"" and got == want


@pytest.fixture(scope="module")
def lib():
    return _load()


def test_split_deflate_hello_world(lib):
    """the reference's split_deflate case: b"Hello World!\\n" in pieces of 6 bytes, gzip, level 6"""
    import zlib_abi_harness as H
    e = _Ctx(lib)
    data = b"Hello World!\n"
    s, idx = e.stream(data, 6, 2)
    d = zlib.decompressobj(31)
    assert d.decompress(s) == data and d.eof and d.unused_data == b""
    assert s[-8:] == zlib.crc32(data).to_bytes(4, "little") + (13).to_bytes(4, "little")
    ref = H.deflate_stream(H.bind(C.CDLL(EMU)), data, level=6, wbits=31)
    assert s[:10] == ref[:10]
    # three pieces, the first two behind their sync markers
    assert len(idx) == 4 and idx[0] == 10 and idx[3] == len(s) - 8
    for i in (1, 2):
        assert s[idx[i] - 4:idx[i]] == MARKER
    e.close()


@pytest.mark.parametrize("level,piece", [(1, 64 << 10), (6, 4 << 10), (9, 16 << 10)])
def test_sizes_matrix_is_one_stream(lib, level, piece):
    e = _Ctx(lib)
    for n in (0, 1, piece - 1, piece, piece + 1, 5 * piece + 17):
        data = _data(n, n + level)
        for wrap in (0, 1, 2):
            for flags in (0, INDEPENDENT):
                s, _ = e.stream(data, piece, wrap, flags, level)
                _one_stream(s, wrap, data)
                if n == 0:
                    h = int(lib.zmi_stream_header_bytes(wrap))
                    assert s[h:h + 2] == b"\x03\x00"
    e.close()


def test_header_matches_library_deflate(lib):
    """zlib FLEVEL / gzip XFL follow level and strategy exactly as this library's deflateInit2_ + deflate() write them"""
    import zlib_abi_harness as H
    abi = H.bind(C.CDLL(EMU))
    e = _Ctx(lib)
    data = _data(3000, 5)
    for level in (0, 1, 2, 5, 6, 7, 9):
        for strategy in (0, 1, 2, 3, 4):
            for wrap in (1, 2):
                s, _ = e.stream(data, 1024, wrap, 0, level, strategy)
                _one_stream(s, wrap, data)
                ref = H.deflate_stream(abi, data, level=level, wbits=WBITS[wrap], strategy=strategy)
                h = int(lib.zmi_stream_header_bytes(wrap))
                assert s[:h] == ref[:h], (level, strategy, wrap)
    e.close()


def test_piece_index(lib):
    e = _Ctx(lib)
    P = 4096
    data = _data(7 * P + 1234, 11)
    pieces = [data[i:i + P] for i in range(0, len(data), P)]
    for wrap in (0, 1, 2):
        h = int(lib.zmi_stream_header_bytes(wrap))
        for flags in (0, INDEPENDENT):
            s, idx = e.stream(data, P, wrap, flags)
            assert len(idx) == len(pieces) + 1 and idx[0] == h
            assert idx[-1] == len(s) - {0: 0, 1: 4, 2: 8}[wrap]
            for i in range(1, len(pieces)):
                assert s[idx[i] - 4:idx[i]] == MARKER
            if flags == INDEPENDENT:
                for i, want in enumerate(pieces):
                    d = zlib.decompressobj(-15)
                    assert d.decompress(s[idx[i]:idx[i + 1]]) == want
                    assert d.eof == (i == len(pieces) - 1)
    e.close()


def test_bad_arguments(lib):
    e = _Ctx(lib)
    buf = np.zeros(4096, dtype=np.uint8)
    w = np.zeros(4, dtype=np.uint64)
    for piece in (0, (1 << 30) + 1):
        assert lib.zmi_deflate_stream_dev(e.ctx, _p(buf), 100, piece, 6, 0, 1, 0, _p(buf), 4096, _p(w), None, _p(w), None) == -103
    assert lib.zmi_deflate_stream_dev(e.ctx, _p(buf), 100, 64, 6, 0, 1, 2, _p(buf), 4096, _p(w), None, _p(w), None) == -103
    assert lib.zmi_deflate_stream_dev(e.ctx, _p(buf), 100, 64, 6, 0, 3, 0, _p(buf), 4096, _p(w), None, _p(w), None) == -103
    # too small an output: Z_BUF_ERROR in the status word, the needed size in the length word, nothing written past the capacity
    data = np.frombuffer(_data(5000, 1) + b"\0" * 16, dtype=np.uint8).copy()
    out = np.full(200, 0x5A, dtype=np.uint8)
    ol = np.zeros(1, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    e.ok(lib.zmi_deflate_stream_dev(e.ctx, _p(data), 5000, 1000, 6, 0, 2, 0, _p(out), 100, _p(ol), None, _p(st), None), "small cap")
    assert int(st[0]) == -5 and int(ol[0]) > 100 and (out[100:] == 0x5A).all()
    e.close()


def _host_fold(sysz, wrap, checks, lens, world, n_local):
    comb = sysz.adler32_combine64 if wrap == 1 else sysz.crc32_combine64
    acc, total = (1 if wrap == 1 else 0), 0
    for g in range(world * n_local):
        k = (g % world) * n_local + g // world
        if lens[k]:
            acc = comb(acc, int(checks[k]), int(lens[k]))
            total += int(lens[k])
    return acc, total


def test_combine_against_system_zlib(lib):
    sysz = C.CDLL("libz.so.1")
    for f in (sysz.crc32_combine64, sysz.adler32_combine64):
        f.restype = C.c_ulong
        f.argtypes = [C.c_ulong, C.c_ulong, C.c_int64]
    e = _Ctx(lib)
    rnd = np.random.default_rng(7)
    for n_entries, world in ((1, 1), (5, 2), (1000, 3), (4096, 1), (4097, 1), (20000, 2), (70000, 1), (69999, 3)):
        n_local = -(-n_entries // world)
        for wrap in (1, 2):
            lens = rnd.integers(0, 1 << 21, size=world * n_local, dtype=np.uint64).astype(np.uint32)
            lens[rnd.random(lens.size) < 0.05] = 0
            lens[rnd.random(lens.size) < 0.02] = 0xFFFFFFFF - rnd.integers(0, 1000, dtype=np.uint32)
            if wrap == 1:   # valid Adler-32 values: both halves below 65521
                checks = (rnd.integers(0, 65521, lens.size, dtype=np.uint32) << 16) | rnd.integers(0, 65521, lens.size, dtype=np.uint32)
            else:
                checks = rnd.integers(0, 1 << 32, lens.size, dtype=np.uint64).astype(np.uint32)
            # padding of the short ranks (and any zero-length entry) counts as nothing whatever its check field holds
            for r in range(world):
                for j in range(n_local):
                    if j * world + r >= n_entries:
                        lens[r * n_local + j] = 0
            checks[lens == 0] = rnd.integers(0, 1 << 32, int((lens == 0).sum()), dtype=np.uint64).astype(np.uint32)
            oc = np.zeros(1, dtype=np.uint32)
            ol = np.zeros(1, dtype=np.uint64)
            e.ok(lib.zmi_checksum_combine_dev(e.ctx, wrap, _p(checks), _p(lens), world, n_local, _p(oc), _p(ol), None), "combine")
            want_c, want_l = _host_fold(sysz, wrap, checks, lens, world, n_local)
            assert int(oc[0]) == want_c and int(ol[0]) == want_l, (n_entries, world, wrap)
            assert want_l > 1 << 32 or n_entries < 4096
    # nothing at all: the identity (Adler-32 1, CRC-32 0)
    oc = np.full(1, 9, dtype=np.uint32)
    ol = np.full(1, 9, dtype=np.uint64)
    e.ok(lib.zmi_checksum_combine_dev(e.ctx, 1, None, None, 1, 0, _p(oc), _p(ol), None), "empty")
    assert int(oc[0]) == 1 and int(ol[0]) == 0
    e.close()


def test_deterministic_across_calls_and_scratch_limits(lib):
    P = 4096
    data = _data(9 * P + 100, 3)
    e = _Ctx(lib)
    runs = {}
    for flags in (0, INDEPENDENT):
        a, ia = e.stream(data, P, 2, flags)
        b, ib = e.stream(data, P, 2, flags)
        assert a == b and ia == ib
        runs[flags] = a
    f = _Ctx(lib)
    f.ok(lib.zmi_ctx_set_scratch_limit(f.ctx, 64 << 20), "scratch limit")
    for flags in (0, INDEPENDENT):
        assert f.stream(data, P, 2, flags)[0] == runs[flags]
    e.close()
    f.close()
    # the launch grouping (a tuning override, read only in a process started with ZMI_TUNING): groups of 1, 2 and 4 pieces give the
    # bytes of the single launch
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "data.npy"), np.frombuffer(data, dtype=np.uint8))
        code = ("import sys, numpy as np; sys.path.insert(0, %r); import test_emu_stream_deflate as T; L = T._load(False); e = T._Ctx(L);"
                "d = bytes(np.load(%r)); open(%r, 'wb').write(b''.join(e.stream(d, %d, 2, f)[0] for f in (0, 1)))") % (
                    os.path.join(ROOT, "tests"), os.path.join(tmp, "data.npy"), os.path.join(tmp, "out"), P)
        for group in ("1", "2", "4"):
            env = dict(os.environ, ZMI_TUNING="1", ZMI_STREAM_GROUP=group)
            r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert open(os.path.join(tmp, "out"), "rb").read() == runs[0] + runs[INDEPENDENT], group


# ---- several ranks: the per-rank building blocks through the exchange (mock RCCL), against one independent-mode call -----------
P_RANK = 4096


def _rank_stream(L, e, comm, rank, world, data, wrap, level):
    """this rank's share of the job -> the stitched stream (every rank receives every slab)"""
    n = len(data)
    np_total = max(1, -(-n // P_RANK))
    max_len = min(P_RANK, n)
    n_local = -(-np_total // world)
    mine = [g for g in range(rank, np_total, world)]
    # independent pieces take any layout: the rank's pieces back to back, each on its own 64-byte line
    offs, lens, buf = [], [], bytearray()
    for g in mine:
        piece = data[g * P_RANK:(g + 1) * P_RANK]
        offs.append(len(buf))
        lens.append(len(piece))
        buf += piece + b"\0" * (-len(piece) % 64)
    inp = np.frombuffer(bytes(buf) + b"\0" * 64, dtype=np.uint8).copy()
    d_off = np.array(offs or [0], dtype=np.uint64)
    d_len = np.array(lens or [0], dtype=np.uint32)
    stride = int(L.zmi_deflate_pieces_stride(max_len))
    slots = np.zeros(max(1, n_local) * stride, dtype=np.uint8)
    sizes = np.zeros(n_local, dtype=np.uint32)       # pad entries stay 0
    checks = np.zeros(n_local, dtype=np.uint32)
    raw = np.zeros(n_local, dtype=np.uint32)
    raw[:len(lens)] = lens
    st = np.zeros(max(1, n_local), dtype=np.int32)
    final = (np_total - 1) % world == rank            # the owner of the last piece ends the stream
    e.ok(L.zmi_deflate_pieces_dev(e.ctx, _p(inp), _p(d_off), _p(d_len), len(mine), max_len, level, 0, wrap, INDEPENDENT, int(final),
                                  _p(slots), stride, _p(sizes), _p(checks), _p(st), None), "zmi_deflate_pieces_dev")
    assert (st == 0).all()
    slab = np.zeros(int(sizes.sum()) + 64, dtype=np.uint8)
    soff_own = np.zeros(n_local + 1, dtype=np.uint64)
    e.ok(L.zmi_pack_slab_dev(e.ctx, _p(slots), stride, _p(sizes), n_local, _p(slab), slab.size, _p(soff_own), None), "pack")
    tables = {}
    for name, a in (("size", sizes), ("check", checks), ("raw", raw)):
        t = np.zeros((world, n_local), dtype=np.uint32)
        e.ok(L.zmi_exchange_sizes(comm, _p(a), n_local, _p(t), None), "zmi_exchange_sizes " + name)
        tables[name] = t
    table = tables["size"]
    goff = np.zeros((world, n_local), dtype=np.uint64)
    soff = np.zeros((world, n_local + 1), dtype=np.uint64)
    d_tot = np.zeros(world + 1, dtype=np.uint64)
    totals = np.zeros(world + 1, dtype=np.uint64)
    e.ok(L.zmi_stitch_plan_dev(e.ctx, _p(table), world, n_local, _p(goff), _p(soff), _p(d_tot), _p(totals), None), "plan")
    recv = [np.zeros(int(totals[p]) + 64, dtype=np.uint8) for p in range(world)]
    ptrs = (C.c_void_p * world)(*[None if p == rank else _p(recv[p]) for p in range(world)])
    e.ok(L.zmi_exchange_slabs(comm, _p(slab), _p(totals), ptrs, 1 << 20, -1, None), "zmi_exchange_slabs")
    h = int(L.zmi_stream_header_bytes(wrap))
    cap = int(L.zmi_deflate_stream_bound(n, P_RANK, wrap))
    out = np.zeros(cap + 64, dtype=np.uint8)
    for r in range(world):
        src = slab if r == rank else recv[r]
        so = soff[r][:-1].copy()
        go = goff[r].copy()
        e.ok(L.zmi_copy_ranges_dev(e.ctx, _p(src), _p(so), 0, _p(table[r]), n_local, max(1, int(table.max())), _p(out) + h, _p(go),
                                   cap - h, None), "scatter")
    chk = np.zeros(1, dtype=np.uint32)
    rawtot = np.zeros(1, dtype=np.uint64)
    if wrap:
        e.ok(L.zmi_checksum_combine_dev(e.ctx, wrap, _p(tables["check"]), _p(tables["raw"]), world, n_local, _p(chk), _p(rawtot), None),
             "combine")
        assert int(rawtot[0]) == n
    olen = np.zeros(1, dtype=np.uint64)
    fst = np.full(1, 7, dtype=np.int32)
    e.ok(L.zmi_stream_frame_dev(e.ctx, wrap, level, 0, _p(d_tot[world:]), _p(chk), _p(rawtot), _p(out), cap, _p(olen), _p(fst), None),
         "frame")
    assert int(fst[0]) == 0
    return bytes(out[:int(olen[0])])


def _rank_worker(rank, world, wire, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["ZMI_RCCL_LIB"] = os.path.join(ROOT, "tests", "emu", "libmock_rccl.so")
        os.environ["ZMI_MOCK_RCCL_DIR"] = wire
        L = _load(False)
        e = _Ctx(L)
        idf = os.path.join(wire, "uid")
        uid = C.create_string_buffer(128)
        if rank == 0:
            e.ok(L.zmi_comm_unique_id(uid), "zmi_comm_unique_id")
            open(idf + ".tmp", "wb").write(uid.raw)
            os.rename(idf + ".tmp", idf)
        else:
            import time
            for _ in range(3000):
                if os.path.exists(idf):
                    break
                time.sleep(0.01)
            uid = C.create_string_buffer(open(idf, "rb").read(), 128)
        comm = C.c_void_p()
        e.ok(L.zmi_comm_create(C.byref(comm), e.ctx, world, rank, uid), "zmi_comm_create")
        # piece counts that do not divide by the world size (padded rows), a short last piece, a single piece
        for n, wrap, level in ((7 * P_RANK + 1000, 2, 6), (8 * P_RANK, 1, 1), (5 * P_RANK + 3, 0, 9), (100, 2, 6)):
            data = _data(n, n)
            got = _rank_stream(L, e, comm, rank, world, data, wrap, level)
            want, _ = e.stream(data, P_RANK, wrap, INDEPENDENT, level)
            assert got == want, (n, wrap, level)
            _one_stream(got, wrap, data)
        e.ok(L.zmi_comm_destroy(comm), "zmi_comm_destroy")
        e.close()
        q.put((rank, "ok"))
    except Exception as ex:  # noqa: BLE001
        import traceback
        q.put((rank, "FAIL " + repr(ex) + "\n" + traceback.format_exc()))


def _run_ranks(world):
    _load()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with tempfile.TemporaryDirectory(prefix="zmi_wire_") as wire:
        procs = [ctx.Process(target=_rank_worker, args=(r, world, wire, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = [q.get(timeout=600) for _ in range(world)]
        for p in procs:
            p.join(60)
    assert sorted(res) == [(r, "ok") for r in range(world)], res


def test_single_stream_two_ranks():
    _run_ranks(2)


def test_single_stream_three_ranks():
    _run_ranks(3)
