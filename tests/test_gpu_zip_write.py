"""The ZIP writer on the MI355X: the checks of tests/zip_write_checks.py over their whole matrices through the library's C ABI on torch
buffers, the archives of 65 534 .. 65 536 entries, and the Engine layer (zip_bound, zip_write, save_npz)."""
import io
import os
import zipfile

import numpy as np
import pytest
import torch

import zip_write_checks as K

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


@pytest.mark.parametrize("level,strategy", K.CONFIGS)
def test_sizes_and_pieces(target, level, strategy):
    """the seven lengths around piece_bytes 4096 as text, mix, zeros and random bytes at the four input alignments"""
    assert K.shapes(target, [(level, strategy)]) == 16


def test_small_pieces(target):
    assert K.small_pieces(target) == 12


def test_many_pieces(target):
    assert K.many_pieces(target) == 2


def test_random_data_expands(target):
    assert K.random_expands(target) == 1


@pytest.mark.parametrize("level", [6, 0])
def test_names(target, level):
    assert K.name_shapes(target, level=level) == 3


@pytest.mark.parametrize("level", [6, 0])
def test_tables(target, level):
    assert K.tables(target, level=level) == 4


def test_grouping(target):
    assert K.grouping(target, _setenv) == 4


def test_zip64_through_base(target):
    assert K.zip64_base(target) == 8


@pytest.mark.parametrize("count", [65534, 65535, 65536])
def test_zip64_through_the_count(target, count):
    assert K.zip64_count(target, [count]) == 1


def test_capacity(target):
    assert K.capacity(target) == 10


def test_arguments(target):
    assert K.arguments(target) == 18 + 2 + 5 + 6 + 2


def test_determinism(target):
    """levels 1 and 3 too (three producer waves in the match search: byte-stable since its producers wait for both chunks a tile reads)"""
    assert K.determinism(target, levels=(0, 1, 3, 6, 9)) == 15


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------
def _entries(e, lens, seed=5):
    raws = K.entries_of("mix", lens, seed)
    data = torch.from_numpy(np.frombuffer(b"".join(raws) + b"\0", dtype=np.uint8).copy()).to(e.device)[:sum(lens)]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]]), dtype=torch.int64, device=e.device)
    return raws, data, off, torch.tensor(lens, dtype=torch.int32, device=e.device)


def test_engine_zip_write_and_read(target, inf_selection):
    e = target.e
    lens = [0, 5000, 1 << 16, 70001, 3]
    names = ["a.txt", "dir/b.bin", "dir/é.dat", "c", "dir/b.bin"]
    raws, data, off, ln = _entries(e, lens)
    enc = [nm.encode("utf-8") for nm in names]
    plain = e.zip_write(data, off, ln, names, piece_bytes=1 << 16)
    K.check_zipfile(plain.cpu().numpy().tobytes(), raws, enc, 8)
    assert int(plain.numel()) <= e.zip_bound(len(lens), sum(map(len, enc)), sum(lens), 1 << 16)
    z, d = e.zip_write(data, off, ln, names, piece_bytes=1 << 16, directory=True)
    assert torch.equal(z, plain)
    assert d.n_entries == len(lens) and d.names() == names and d.index("dir/b.bin") == 4 and bool(d.readable.all())
    want = e.zip_directory(z)
    assert torch.equal(d.entries, want.entries) and d.info == want.info
    out, ooff, olen, st = e.zip_read(z, d, names=["dir/é.dat", "a.txt", "c"])
    torch.cuda.synchronize()
    assert st.tolist() == [0, 0, 0] and olen.tolist() == [lens[2], 0, lens[3]]
    host, o = out.cpu().numpy().tobytes(), ooff.tolist()
    assert host[o[0]:o[1]] == raws[2] and host[o[2]:o[3]] == raws[3]
    # names as a (blob, offsets) pair, level 0, and the two tables
    blob = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy()).to(e.device)
    noff = torch.tensor(np.concatenate([[0], np.cumsum([len(b) for b in enc])]), dtype=torch.int64, device=e.device)
    dos = torch.tensor([0x58A1B8C2] * 5, dtype=torch.int32, device=e.device)
    ext = torch.from_numpy(np.array([0o100600 << 16] * 5, dtype=np.uint32).view(np.int32)).to(e.device)
    s, ds = e.zip_write(data, off, ln, (blob, noff), level=0, dos_time=dos, ext_attr=ext, directory=True)
    K.check_zipfile(s.cpu().numpy().tobytes(), raws, enc, 0, dos=[0x58A1B8C2] * 5, ext=[0o100600 << 16] * 5)
    out, ooff, olen, st = e.zip_read(s, ds)
    assert st.tolist() == [0] * 5 and out.cpu().numpy().tobytes() == b"".join(raws)


def test_engine_zip_write_raises_where_out_is_too_small(target):
    e = target.e
    raws, data, off, ln = _entries(e, [3000, 100])
    whole = e.zip_write(data, off, ln, ["x", "y"])
    with pytest.raises(RuntimeError, match=r"zmi_zip_write_dev: status -5 \(archive of %d bytes, room for %d\)" % (whole.numel(), whole.numel() - 1)):
        e.zip_write(data, off, ln, ["x", "y"], out=torch.empty(int(whole.numel()) - 1, dtype=torch.uint8, device=e.device))
    assert torch.equal(e.zip_write(data, off, ln, ["x", "y"], out=torch.empty(int(whole.numel()), dtype=torch.uint8, device=e.device)), whole)
    with pytest.raises(ValueError):
        e.zip_write(data, off, ln, ["x"])


def test_engine_zip_write_converts_its_tables(target):
    """tables and the names blob on the host, of another integer type or strided give the same archive; data is never copied"""
    e = target.e
    lens = [700, 0, 5000]
    raws, data, off, ln = _entries(e, lens)
    enc = [b"one", b"", b"dir/three"]
    blob = torch.from_numpy(np.frombuffer(b"".join(enc), dtype=np.uint8).copy())
    noff = torch.tensor([0, 3, 3, 12], dtype=torch.int32)
    for level in (6, 0):
        want = e.zip_write(data, off, ln, (blob.to(e.device), noff.to(e.device)), level=level, piece_bytes=4096)
        K.check_zipfile(want.cpu().numpy().tobytes(), raws, enc, 8 if level else 0)
        wide = torch.stack([ln.to(torch.int64), ln.to(torch.int64)], dim=1)[:, 0]          # int64 and strided
        got = e.zip_write(data, off.cpu().to(torch.int32), wide, (blob, noff), level=level, piece_bytes=4096)
        assert torch.equal(got, want)
    with pytest.raises(ValueError, match="data must be a contiguous uint8 tensor"):
        e.zip_write(data.cpu(), off, ln, ["a", "b", "c"])
    with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor"):
        e.zip_write(data, off, ln, ["a", "b", "c"], out=torch.empty(1 << 16, dtype=torch.uint8))


@pytest.mark.parametrize("level", [6, 0, -1])
def test_engine_empty_archive(target, level):
    e = target.e
    none = torch.empty(0, dtype=torch.uint8, device=e.device)
    z = e.zip_write(none, torch.empty(0, dtype=torch.int64, device=e.device), torch.empty(0, dtype=torch.int32, device=e.device), [], level=level)
    assert z.cpu().numpy().tobytes() == K.EMPTY
    blob = e.save_npz({}, level=level)
    assert blob == K.EMPTY
    with np.load(io.BytesIO(blob)) as f:
        assert f.files == []


@pytest.mark.parametrize("level", [6, 0])
def test_engine_save_npz(target, level):
    e = target.e
    g = torch.Generator().manual_seed(3)
    arrays = {"w": torch.randn(300, 70, generator=g), "idx": torch.arange(-5, 4000, dtype=torch.int64), "flag": torch.tensor([True, False, True]),
              "half": torch.randn(17, generator=g).to(torch.float16), "bytes": torch.arange(256, dtype=torch.uint8).reshape(4, 8, 8),
              "scalar": torch.tensor(2.5, dtype=torch.float64), "empty": torch.zeros((0, 3), dtype=torch.int16),
              "strided": torch.arange(60, dtype=torch.int32).reshape(6, 10).t(), "small": torch.tensor([-3, 7], dtype=torch.int8)}
    blob = e.save_npz({k: v.to(e.device) for k, v in arrays.items()}, level=level, piece_bytes=1 << 14)
    with np.load(io.BytesIO(blob)) as z:
        assert sorted(z.files) == sorted(arrays)
        for k, v in arrays.items():
            got = z[k]
            assert got.dtype == v.numpy().dtype and got.shape == tuple(v.shape) and np.array_equal(got, v.numpy()), k
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        assert zf.testzip() is None and all(zi.compress_type == (8 if level else 0) for zi in zf.infolist())
    # the library's own reader returns the .npy files
    d = e.zip_directory(blob)
    out, ooff, olen, st = e.zip_read(d.data, d)
    assert d.names() == [k + ".npy" for k in arrays] and not st.any()
    host, o = out.cpu().numpy().tobytes(), ooff.tolist()
    for j, (k, v) in enumerate(arrays.items()):
        buf = io.BytesIO()
        np.save(buf, np.asarray(v.numpy(), order="C"))
        assert host[o[j]:o[j] + int(olen[j])] == buf.getvalue(), k
    with pytest.raises(TypeError, match="bfloat16"):
        e.save_npz({"b": torch.zeros(4, dtype=torch.bfloat16, device=e.device)})
