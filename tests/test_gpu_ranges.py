"""zmi_inflate_stream_index_dev / zmi_inflate_ranges_dev on the MI355X: the checks of tests/ranges_checks.py over their whole matrices
through the library's C ABI on torch buffers, under both decode-kernel selections, then the Engine layer (inflate_stream_indexed,
StreamIndex.save / load / from_pieces, read_ranges)."""
import gzip
import os
import random

import numpy as np
import pytest
import torch

import ranges_checks as K

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
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = GpuTarget()
    yield t
    t.e.close()


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


@pytest.mark.parametrize("name", ["F1-gzip", "F2", "F4", "F5"])
def test_index_is_exact(target, inf_selection, name):
    assert K.index_exact(target, name, setenv=_setenv) == 4 + 3 + 3


def test_void_index(target, inf_selection):
    assert K.void_index(target) == 3


@pytest.mark.parametrize("span", [1, 40000])
@pytest.mark.parametrize("name", ["F1-raw", "F1-zlib", "F1-gzip", "F2"])
def test_ranges_are_exact(target, inf_selection, name, span):
    assert K.ranges_exact(target, name, span) == 59 * 3


@pytest.mark.parametrize("name,span", [("F1-gzip", 40000), ("F2", 1)])
def test_independence(target, inf_selection, name, span):
    assert K.independence(target, name, span) == 4


def test_windows_matter_and_may_be_withheld(target, inf_selection):
    assert K.windows(target) == 7


def test_truncation(target, inf_selection):
    assert K.truncation(target) == 4


@pytest.mark.parametrize("jump", ["0", "1"])
def test_a_few_ranges_under_either_resolve(target, monkeypatch, jump):
    """a launch of up to 16 ranges may take the pointer-jumping resolve: the same results from it and from the serial pass"""
    monkeypatch.setenv("ZMI_INF_JUMP", jump)
    assert K.windows(target) == 7 and K.truncation(target) == 4


def test_arguments(target):
    assert K.arguments(target) == 12 + 6 + 7


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------
def _dev(target, b):
    return target.mem.put(np.frombuffer(bytes(b) + b"\0" * 16, dtype=np.uint8)).t[:len(b)]


def _check_reads(e, stream, index, payload, ranges):
    lo = [a for a, _ in ranges]
    ln = [b for _, b in ranges]
    out, got, st = e.read_ranges(stream, index, lo, ln)
    host, got, st = out.cpu().numpy(), got.tolist(), st.tolist()
    for i, (a, b) in enumerate(ranges):
        want = payload[a:a + b]
        assert (got[i], st[i]) == (len(want), 0) and host[i, :got[i]].tobytes() == want, (i, a, b, got[i], st[i])


def test_from_pieces_reads_an_independent_stream_without_windows(target, inf_selection):
    e, data = target.e, K.data()
    stream, idx = e.deflate_stream(_dev(target, data), wrap=K.GZIP, piece_bytes=16384, independent=True, index=True)
    from zlib_rs_amd.engine import StreamIndex
    index = StreamIndex.from_pieces(idx, 16384, len(data))
    assert index.win is None and index.n_points == 10 and index.out.tolist() == [16384 * i for i in range(10)] + [len(data)]
    total = len(data)
    ranges = [(0, 1), (0, total), (total - 1, 1), (total, 5), (total - 3, 10), (16384, 1), (16383, 2), (7, 0)] + K.seeded_ranges(total, 50)
    _check_reads(e, stream, index, data, ranges)


def _words_text(n, seed):
    rnd = random.Random(seed)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(2000)]
    pick = np.random.RandomState(seed).randint(0, len(words), size=n // 5)
    return b" ".join(words[i] for i in pick)[:n]


@pytest.fixture(scope="module")
def big_text():
    return _words_text(8 << 20, 11)


def _engine_round(target, tmp_path, stream_dev, payload, bit_cuts=None):
    from zlib_rs_amd.engine import StreamIndex
    e = target.e
    out, used, index = e.inflate_stream_indexed(stream_dev, bit_cuts=bit_cuts, span=1 << 20)
    assert used == stream_dev.numel() and out.cpu().numpy().tobytes() == payload
    offs = index.out.tolist()
    assert offs[0] == 0 and offs[-1] == len(payload) and 3 <= index.n_points <= 9 and all(b - a >= 1 << 20 for a, b in zip(offs, offs[1:-1]))
    assert index.max_gap == max(b - a for a, b in zip(offs, offs[1:])) and tuple(index.win.shape) == (index.n_points, 32768)
    path = str(tmp_path / "index.npz")
    index.save(path)
    back = StreamIndex.load(path, e.device)
    assert back.max_gap == index.max_gap and torch.equal(back.bit, index.bit) and torch.equal(back.out, index.out) and torch.equal(back.win, index.win)
    r = random.Random(3)
    ranges = [(r.randrange(0, len(payload)), r.randint(1, 65536)) for _ in range(256)]
    _check_reads(e, stream_dev, back, payload, ranges)
    # into a buffer of the caller's with an offset table: no synchronisation, nothing outside the ranges written
    lo = torch.tensor([a for a, _ in ranges], dtype=torch.int64, device=e.device)
    ln = torch.tensor([b for _, b in ranges], dtype=torch.int32, device=e.device)
    offs_out = torch.arange(256, dtype=torch.int64, device=e.device) * 65600 + 1
    buf = torch.full((256 * 65600 + 1,), 0xA5, dtype=torch.uint8, device=e.device)
    _, got, st = e.read_ranges(stream_dev, back, lo, ln, out=buf, out_offsets=offs_out, max_len=65536)
    host, got = buf.cpu().numpy(), got.tolist()
    assert st.tolist() == [0] * 256
    for i, (a, b) in enumerate(ranges):
        o = 1 + 65600 * i
        assert host[o:o + got[i]].tobytes() == payload[a:a + b] and (host[o + got[i]:o + 65600] == 0xA5).all(), i


def test_engine_on_a_gzip_stream(target, inf_selection, tmp_path, big_text):
    _engine_round(target, tmp_path, _dev(target, gzip.compress(big_text, 6)), big_text)


def test_engine_on_a_carry_stream(target, inf_selection, tmp_path, big_text):
    e = target.e
    stream = e.deflate_stream(_dev(target, big_text), wrap=K.GZIP)
    _engine_round(target, tmp_path, stream, big_text, bit_cuts=8 * e.find_cuts(stream, K.GZIP))


def test_engine_on_the_empty_stream(target):
    import zlib
    e = target.e
    s = _dev(target, zlib.compress(b""))
    out, used, index = e.inflate_stream_indexed(s)
    assert out.numel() == 0 and used == 8 and index.n_points == 1 and index.out.tolist() == [0, 0] and index.max_gap == 0
    out, got, st = e.read_ranges(s, index, [0, 0, 5, 1 << 40], [0, 1, 100, 7])
    assert got.tolist() == [0] * 4 and st.tolist() == [0] * 4
