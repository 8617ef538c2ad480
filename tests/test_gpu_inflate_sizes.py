"""zmi_inflate_sizes_dev / zmi_inflate_batch_packed_dev on the MI355X: the two calls go through Engine (inflate_sizes,
inflate_batch_packed with `out` given), the judge zmi_inflate_batch_dev_ex through the same library's C ABI; the checks are those of
tests/inflate_sizes_checks.py over their whole matrices, under both decode-kernel selections."""
import numpy as np
import pytest
import torch

import inflate_sizes_checks as K

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


class GpuTarget(K.AbiTarget):
    def __init__(self):
        from zlib_rs_amd.engine import Engine
        self.e = Engine(0)
        super().__init__(self.e.L, self.e._ctx, TorchMem(self.e.device))

    def close(self):
        self.e.close()

    @staticmethod
    def _typed(h, n, dtype):
        return h.t[:n * dtype.itemsize].view(dtype)

    def _sizes(self, d, off, ln, n, wrap, hist, limit, size, st, used, det):
        i32, i64 = torch.int32, torch.int64
        sizes, status = self.e.inflate_sizes(d.t, self._typed(off, n, i64), self._typed(ln, n, i32), wrap=wrap, hist=hist, size_limit=limit,
                                             in_used=self._typed(used, n, i32), detail=self._typed(det, n, i32))
        self._typed(size, n, i32).copy_(sizes)
        self._typed(st, n, i32).copy_(status)

    def _packed(self, d, off, ln, n, wrap, zd, zlen, limit, align, out, out_cap, ooff, olen, st, used, det):
        i32, i64 = torch.int32, torch.int64
        o, ooffs, lens, status = self.e.inflate_batch_packed(d.t, self._typed(off, n, i64), self._typed(ln, n, i32), wrap=wrap,
                                                             zdict=zd.t[:zlen] if zd is not None else None, size_limit=limit, align=align,
                                                             out=out.t[:out_cap], in_used=self._typed(used, n, i32), detail=self._typed(det, n, i32))
        self._typed(ooff, n + 1, i64).copy_(ooffs)
        self._typed(olen, n, i32).copy_(lens)
        self._typed(st, n, i32).copy_(status)
        return 0

    def own(self, shards, level, wrap):
        lens = [len(s) for s in shards]
        off = np.zeros(len(shards), dtype=np.int64)
        off[1:] = np.cumsum(lens[:-1])
        dev = self.e.device
        data = self.mem.put(np.frombuffer(b"".join(shards) + b"\0", dtype=np.uint8)).t
        out, olen, st = self.e.deflate_batch(data, torch.from_numpy(off).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), max(lens),
                                             level=level, wrap=wrap)
        assert (st.cpu().numpy() == 0).all()
        host, n = out.cpu().numpy(), olen.cpu().numpy()
        return [host[i, :n[i]].tobytes() for i in range(len(shards))]


@pytest.fixture(scope="module")
def target():
    t = GpuTarget()
    yield t
    t.close()


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_sizes_are_exact(target, inf_selection, wrap):
    assert K.sizes_exact(target, wrap) == 7 * len(K.LENS) + 9


def test_sizes_of_many_tiny_streams(target, inf_selection):
    assert K.sizes_many_tiny(target) == 600


def test_sizes_of_own_output(target, inf_selection):
    assert K.sizes_own_output(target) == 45


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_independence(target, inf_selection, wrap):
    assert K.independence(target, wrap) >= 25


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_failing_streams(target, inf_selection, wrap):
    assert K.failing_streams(target, wrap) >= 9


def test_history(target, inf_selection):
    assert K.history(target) == 5


def test_wrong_check_values(target, inf_selection):
    assert K.wrong_checks(target) == 3


def test_size_limit(target, inf_selection):
    assert K.size_limit(target) == 7


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB, K.GZIP, K.AUTO])
def test_packed_equals_batch(target, inf_selection, wrap, align):
    assert K.packed_equals_batch(target, wrap, align) == 7 * len(K.LENS) + 9


def test_packed_with_a_shared_dictionary(target, inf_selection):
    assert K.packed_shared_dict(target) == 13


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(target, inf_selection, align):
    assert K.capacity(target, align=align) == 4


def test_arguments(target):
    assert K.arguments(target) == 17


def test_context_limit_is_the_callers(target):
    assert K.context_limit(target) == 4


def test_engine_allocates_exactly(target, inf_selection):
    """Engine.inflate_batch_packed(out=None): one buffer of exactly the planned size whose slices are the payloads; inflate_sizes agrees"""
    e, dev = target.e, target.e.device
    raws = [K.text(n, 90 + n) for n in (0, 1, 300, 4097, 70000, 300000)]
    for wrap, align, zd in ((K.ZLIB, 1, None), (K.GZIP, 16, None), (K.RAW, 1, None), (K.ZLIB, 16, K.text(2000, 5))):
        streams = [K.deflate(r, wrap, (0, 1, 6)[i % 3], zdict=zd) for i, r in enumerate(raws)]
        d, off, ln = target._input(streams)
        n = len(streams)
        offs, lens = target._typed(off, n, torch.int64), target._typed(ln, n, torch.int32)
        zdt = target.mem.put(np.frombuffer(zd, dtype=np.uint8)).t if zd else None
        out, ooff, olen, st = e.inflate_batch_packed(d.t, offs, lens, wrap=wrap, zdict=zdt, align=align)
        want = K.aligned_scan([len(r) for r in raws], align)
        assert ooff.tolist() == want and out.numel() == want[-1] and st.tolist() == [0] * n and olen.tolist() == [len(r) for r in raws]
        host = out.cpu().numpy().tobytes()
        assert [host[want[i]:want[i] + len(r)] for i, r in enumerate(raws)] == raws
        sizes, sst = e.inflate_sizes(d.t, offs, lens, wrap=wrap, hist=len(zd) if zd else 0)
        assert sizes.tolist() == olen.tolist() and sst.tolist() == [0] * n
    out, ooff, olen, st = e.inflate_batch_packed(torch.zeros(16, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                                                 torch.zeros(0, dtype=torch.int32, device=dev))
    assert out.numel() == 0 and ooff.tolist() == [0]
