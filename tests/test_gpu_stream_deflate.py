"""Single-stream (pigz-style) deflate on the MI355X: Engine.deflate_stream / zmi_deflate_stream_dev, the piece index as restart points of
zmi_inflate_split, a stream above 4 GiB (ISIZE wraps), and the single-stream stitch through the real RCCL at world 1.  The contract is
the reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221: one stream, read back whole by the host's zlib."""
import zlib

import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20
WBITS = {0: -15, 1: 15, 2: 31}
TRAILER = {0: 0, 1: 4, 2: 8}


def _one_stream(s, wrap, want):
    d = zlib.decompressobj(WBITS[wrap])
    got = d.decompress(s)
    assert d.eof and d.unused_data == b"" and got == want


@pytest.fixture(scope="module")
def env():
    import torch
    from zlib_rs_amd.engine import Engine
    e = Engine(0)
    data = e.gen_shards(256, MiB)
    torch.cuda.synchronize()
    yield e, data, bytes(data.cpu().numpy())
    e.close()


def test_256mib_one_stream_per_wrap_and_mode(env):
    import torch
    from zlib_rs_amd.engine import uniform_layout
    e, data, host = env
    n_pieces = 256
    off, ln = uniform_layout(n_pieces, MiB, e.device)
    for wrap in (0, 1, 2):
        sizes = {}
        for independent in (False, True):
            s = e.deflate_stream(data, level=6, wrap=wrap, independent=independent)
            torch.cuda.synchronize()
            sizes[independent] = int(s.numel())
            _one_stream(bytes(s.cpu().numpy()), wrap, host)
        assert sizes[False] <= sizes[True], (wrap, sizes)
        # independent pieces are the batch API's members without their wrappers, plus a flush marker behind every piece but the last
        _, olen, st = e.deflate_batch(data, off, ln, MiB, level=6, wrap=wrap)
        torch.cuda.synchronize()
        assert int((st != 0).sum().item()) == 0
        h, t = e.stream_header_bytes(wrap), TRAILER[wrap]
        members = int(olen.to(torch.int64).sum().item()) - n_pieces * (h + t) + 5 * (n_pieces - 1) + h + t
        assert abs(sizes[True] - members) <= 0.002 * members, (wrap, sizes[True], members)


def test_piece_index_feeds_inflate_split(env):
    import torch
    import zmi_ctypes
    e, data, host = env
    lib = zmi_ctypes.load_product()
    z = zmi_ctypes.Engine(lib)
    for independent in (False, True):
        s, idx = e.deflate_stream(data, level=6, wrap=2, index=True, independent=independent)
        torch.cuda.synchronize()
        s = bytes(s.cpu().numpy())
        idx = [int(x) for x in idx.cpu().numpy()]
        h = e.stream_header_bytes(2)
        assert idx[0] == h and idx[-1] == len(s) - 8 and len(idx) == 257
        body = s[h:idx[-1]]
        seg = [x - h for x in idx[:-1]]
        out, st, det, used, res, nused = z.inflate_split(body, seg, cap=len(host) + 4096)
        assert st == 0 and res[3] == 1 and nused == len(seg) and used == len(body), (st, det, nused, used, res)
        assert out == host
    z.close()


def test_stream_above_4gib(env):
    """4 GiB + 3 MiB: three launch groups under the default scratch limit, ISIZE wraps, the CRC trailer equals the host's"""
    import torch
    e, _, _ = env
    n_mib = 4096 + 3
    big = e.gen_shards(n_mib, MiB)
    s = e.deflate_stream(big, level=6, wrap=2)
    torch.cuda.synchronize()
    comp = s.cpu().numpy()
    del s
    total = n_mib * MiB
    assert int.from_bytes(comp[-4:].tobytes(), "little") == total % (1 << 32)
    crc = 0
    pos = 0
    d = zlib.decompressobj(31)

    def consume(got):
        nonlocal crc, pos
        want = bytes(big[pos:pos + len(got)].cpu().numpy())
        assert got == want, pos
        crc = zlib.crc32(want, crc)
        pos += len(got)

    for lo in range(0, comp.size, 64 * MiB):
        consume(d.decompress(comp[lo:lo + 64 * MiB].tobytes()))
    consume(d.flush())
    assert d.eof and d.unused_data == b"" and pos == total
    assert int.from_bytes(comp[-8:-4].tobytes(), "little") == crc
    del big
    torch.cuda.empty_cache()


def test_single_stream_stitch_real_rccl_world1(env):
    import torch
    from zlib_rs_amd import dist
    from zlib_rs_amd.engine import uniform_layout
    e, data, host = env
    n = 64 * MiB + 12345
    part = data[:n]
    P = MiB
    n_pieces = -(-n // P)
    off, ln = uniform_layout(n_pieces, P, e.device)
    ln[-1] = n - (n_pieces - 1) * P
    comm = e.comm_create(1, 0, e.comm_unique_id())
    for wrap in (0, 1, 2):
        slots, sizes, checks, st = e.deflate_pieces(part, off, ln, P, level=6, wrap=wrap, independent=True, final=True)
        slab, _ = e.pack_slab(slots, sizes)
        size_table = e.exchange_sizes(comm, sizes, 1)
        check_table = e.exchange_sizes(comm, checks, 1)
        raw_table = e.exchange_sizes(comm, ln, 1)
        torch.cuda.synchronize()
        assert int((st != 0).sum().item()) == 0
        got, length = dist.stitch_single_stream_on_device(e, [slab], size_table, check_table, raw_table, 6, 0, wrap)
        want = e.deflate_stream(part, level=6, wrap=wrap, independent=True)
        torch.cuda.synchronize()
        assert length == int(want.numel()) and torch.equal(got, want), wrap
        _one_stream(bytes(got.cpu().numpy()), wrap, host[:n])
    e.comm_destroy(comm)
