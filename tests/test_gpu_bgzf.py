"""The BGZF writer on the MI355X: the checks of tests/bgzf_checks.py over their whole matrices through the library's C ABI on torch
buffers, then the Engine layer (bgzf_compress, bgzf_blocks, BgzfIndex with its .gzi files and virtual offsets, bgzf_read_ranges under
both decode-kernel selections, and the library's own readers on the files)."""
import gzip
import os
import struct

import numpy as np
import pytest
import torch

import bgzf_checks as K

pytestmark = pytest.mark.gpu


class TorchMem:
    def __init__(self, device):
        self.device = device

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    class Handle:
        def __init__(self, t):
            self.t, self.ptr = t, t.data_ptr()

    def put(self, arr, shift=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf = torch.zeros(b.size + 32, dtype=torch.uint8, device=self.device)
        at = (shift - buf.data_ptr()) % 16
        view = buf[at:at + b.size]
        if b.size:
            view.copy_(torch.from_numpy(b.copy()))
        return self.Handle(view)

    def full(self, nbytes, fill):
        return self.Handle(torch.full((nbytes,), fill, dtype=torch.uint8, device=self.device))

    def read(self, h, dtype):
        return h.t.cpu().numpy().view(dtype)


class GpuTarget(K.Target):
    def __init__(self):
        from zlib_rs_amd.engine import Engine
        self.e = Engine(0)
        super().__init__(self.e.L, self.e._ctx, TorchMem(self.e.device))


@pytest.fixture(scope="module")
def target():
    t = GpuTarget()
    yield t
    t.e.close()


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("config", K.CONFIGS)
def test_shapes(target, config, kind):
    """8 sizes x 3 block sizes and 3 sizes at block size 1, each at four alignments"""
    assert K.shapes(target, configs=[config], kinds=[kind]) == (8 * 3 + 3) * 4


def test_limit_and_fallback(target):
    assert K.fallback(target) == 2 * 6 * 6


def test_index_is_optional(target):
    assert K.index_optional(target) == 2


def test_grouping(target):
    assert K.grouping(target, _setenv) == 10


def test_empty_shards(target):
    assert K.empty_shards(target) == 4


def test_capacity(target):
    assert K.capacity(target) == 9


def test_arguments(target):
    assert K.arguments(target) == 21 + 3


def test_own_readers(target):
    assert K.own_readers(target) == 2


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------
def _dev(target, b):
    return target.mem.put(np.frombuffer(bytes(b) + b"\0" * 16, dtype=np.uint8), 3).t[:len(b)]


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("bb", [65280, 777])
def test_engine_compress(target, bb):
    e = target.e
    data = K.make("mix", 3 * 65280 + 17 if bb == 65280 else 9 * 777 + 1, bb)
    want = target.deflate(data, bb)
    offs, _ = K.check_file(want, data, bb)
    file, index = e.bgzf_compress(_dev(target, data), block_bytes=bb, index=True)
    assert _host(file) == want.file and gzip.decompress(_host(file)) == data
    assert (index.block_off.tolist(), index.block_bytes, index.n, index.n_blocks) == (offs, bb, len(data), len(offs) - 1)
    assert e.bgzf_bound(len(data), bb) == K.bound(len(data), bb) and e.bgzf_bound(len(data)) == K.bound(len(data), 65280)
    assert _host(e.bgzf_compress(_dev(target, data), block_bytes=bb)) == want.file
    for level, strategy in ((9, 0), (6, 3)):
        assert _host(e.bgzf_compress(_dev(target, data), level, strategy, bb)) == target.deflate(data, bb, level, strategy).file
    small = torch.empty(want.total - 1, dtype=torch.uint8, device=e.device)
    with pytest.raises(RuntimeError, match="status -5"):
        e.bgzf_compress(_dev(target, data), block_bytes=bb, out=small)
    empty = e.bgzf_compress(torch.empty(0, dtype=torch.uint8, device=e.device))
    assert _host(empty) == K.EOF


def test_engine_blocks(target):
    e, bb = target.e, 4096
    data = K.make("mix", 9 * bb + 100, bb)
    shards = K.cut(data, bb)
    want = target.deflate(data, bb)
    offs, _ = K.check_file(want, data, bb)
    d = _dev(target, data)
    off = torch.arange(len(shards), dtype=torch.int64, device=e.device) * bb
    ln = torch.tensor([len(s) for s in shards], dtype=torch.int32, device=e.device)
    slab, block_off, block_len = e.bgzf_blocks(d, off, ln, bb)
    assert _host(slab) + K.EOF == want.file and block_off.tolist() == offs
    assert block_len.tolist() == [b - a for a, b in zip(offs, offs[1:])]
    a, _, la = e.bgzf_blocks(d, off[:4], ln[:4], bb)
    b, _, lb = e.bgzf_blocks(d, off[4:], ln[4:], bb)
    assert _host(a) + _host(b) == _host(slab) and la.tolist() + lb.tolist() == block_len.tolist()
    with pytest.raises(RuntimeError, match="status -103"):
        e.bgzf_blocks(d, off, ln, bb - 1)
    none, o, l = e.bgzf_blocks(d, off[:0], ln[:0], bb)
    assert none.numel() == 0 and o.tolist() == [0] and l.numel() == 0


def test_engine_readers_take_the_index(target, inf_selection):
    e, bb = target.e, 4096
    data = K.make("text", 20 * bb + 5, bb)
    file, index = e.bgzf_compress(_dev(target, data), block_bytes=bb, index=True)
    assert e.find_members(file).tolist() == index.block_off.tolist()
    out, moff = e.inflate_members(file, starts=index.block_off, index=True)
    assert _host(out) == data and e.last_members_in_used == file.numel()
    assert moff.tolist() == [i * bb for i in range(21)] + [len(data), len(data)]


def _ranges(n, bb):
    r = [(5, 100), (bb - 50, 100), (bb - 50, bb + 100), (bb - 1, 2 * bb + 2), (2 * bb + 9, 3 * bb), (bb, bb), (3 * bb, 2 * bb), (0, bb),
         (bb - 10, 10), (bb, 1), (n - 7, 7), (n - 1, 1), (n - 5, 100), (bb + 3, n), (17, 0), (n, 0), (n, 10), (n + 1000, 5), (0, 1)]
    rnd = np.random.RandomState(7)
    return r + [(int(rnd.randint(0, n)), int(rnd.randint(1, 3 * bb))) for _ in range(12)]


@pytest.mark.parametrize("bb,n", [(4096, 10 * 4096 + 123), (777, 40 * 777), (65280, 3 * 65280 + 17)])
def test_read_ranges(target, inf_selection, bb, n):
    """ranges inside one block, across 1, 2 and 3 boundaries, from and to a boundary exactly, the last bytes, past the end (cut), of
    length 0 and behind the data, against slices of the data; nothing outside a range's bytes is written"""
    e = target.e
    data = K.make("mix", n, bb)
    file, index = e.bgzf_compress(_dev(target, data), block_bytes=bb, index=True)
    ranges = _ranges(n, bb)
    lo, ln = [a for a, _ in ranges], [b for _, b in ranges]
    width = max(ln)
    for as_tensor in (False, True):
        buf = torch.full((len(ranges), width), 0xA5, dtype=torch.uint8, device=e.device)
        if as_tensor:
            out, got, st = e.bgzf_read_ranges(file, index, torch.tensor(lo, dtype=torch.int64, device=e.device),
                                              torch.tensor(ln, dtype=torch.int32, device=e.device), out=buf)
        else:
            out, got, st = e.bgzf_read_ranges(file, index, lo, ln, out=buf)
        host, got = out.cpu().numpy(), got.tolist()
        assert st.tolist() == [0] * len(ranges)
        for i, (a, b) in enumerate(ranges):
            want = data[a:a + b]
            assert got[i] == len(want) and host[i, :got[i]].tobytes() == want and (host[i, got[i]:] == 0xA5).all(), (i, a, b, got[i])
    out, got, st = e.bgzf_read_ranges(file, index, lo[:3], ln[:3])         # the buffer allocated by the call
    assert tuple(out.shape) == (3, max(ln[:3])) and got.tolist() == ln[:3]
    assert [out[i, :ln[i]].cpu().numpy().tobytes() for i in range(3)] == [data[a:a + b] for a, b in ranges[:3]]


def test_read_ranges_of_the_empty_file(target):
    e = target.e
    file, index = e.bgzf_compress(torch.empty(0, dtype=torch.uint8, device=e.device), index=True)
    assert (index.n, index.n_blocks, index.block_off.tolist()) == (0, 0, [0])
    out, got, st = e.bgzf_read_ranges(file, index, [0, 5], [0, 9])
    assert got.tolist() == [0, 0] and st.tolist() == [0, 0]


def test_gzi_files_and_virtual_offsets(target, tmp_path):
    from zlib_rs_amd.engine import BgzfIndex
    e, bb = target.e, 4096
    data = K.make("mix", 6 * bb + 31, bb)
    file, index = e.bgzf_compress(_dev(target, data), block_bytes=bb, index=True)
    offs, _, _ = K.walk(_host(file))
    path = str(tmp_path / "a.gzi")
    index.save_gzi(path)
    assert open(path, "rb").read() == struct.pack("<Q", 6) + b"".join(struct.pack("<QQ", offs[i], i * bb) for i in range(1, 7))
    for src in (file, _host(file)):
        back = BgzfIndex.load_gzi(path, src, e.device)
        assert (back.block_bytes, back.n, back.block_off.tolist()) == (bb, len(data), offs) and back.block_off.device == file.device
    for u in (0, 1, bb - 1, bb, 4 * bb + 9, len(data) - 1):
        assert index.virtual_offset(u) == offs[u // bb] << 16 | u % bb == back.virtual_offset(u)
    out, got, st = e.bgzf_read_ranges(file, back, [bb - 3], [2 * bb])      # the loaded index reads
    assert got.tolist() == [2 * bb] and _host(out[0]) == data[bb - 3:3 * bb - 3]
