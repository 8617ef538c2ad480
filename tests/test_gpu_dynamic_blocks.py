"""The decode kernels on hand-built dynamic-Huffman blocks on the MI355X: the checks of tests/dynamic_block_checks.py (48-bit tokens,
tables of exactly 852 and 400 entries, the single-code forms, every header shape, 300 tiny blocks, deliberately placed errors)
through Engine.inflate_batch, the size pass and the packed decode, zmi_inflate_resume / zmi_inflate_blocks (host buffers through the
C ABI), the block scan and zmi_inflate_stream_bits_dev, under both decode-kernel selections.  The hardware path differs from the
emulator's (tests/test_emu_dynamic_blocks.py) in inf_walk and in the alignbit / bit-field instructions with zero widths; the judge
is the oracle and deflate_craft.inflate_ref (tests/test_deflate_craft.py), never the library."""
import ctypes as C

import numpy as np
import pytest

import dynamic_block_checks as K
from test_emu_stream_inflate_blocks import _Ctx, _bind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def o():
    import oracle_lib
    return oracle_lib.load(rebuild=False)


@pytest.fixture(scope="module")
def target():
    from test_gpu_inflate_sizes import GpuTarget
    t = GpuTarget()
    yield t
    t.close()


@pytest.fixture(scope="module")
def eng():
    import zmi_ctypes
    e = zmi_ctypes.Engine(zmi_ctypes.load_product())
    yield e
    e.close()


class GpuCtx(_Ctx):
    """the _Ctx of tests/test_emu_stream_inflate_blocks.py over device memory"""
    def _dev(self, arr):
        import torch
        return torch.from_numpy(arr).to("cuda:0")

    def _find(self, fn, s, wrap, min_gap, cap):
        import torch
        inp = self._dev(np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy())
        cuts = self._dev(np.zeros(max(cap, 1), dtype=np.int64))
        cnt = self._dev(np.full(1, -1, dtype=np.int32))
        self.ok(fn(self.ctx, inp.data_ptr(), len(s), wrap, min_gap, cuts.data_ptr(), cap, cnt.data_ptr(), None), "find")
        torch.cuda.synchronize()
        n = int(cnt.cpu().numpy().view(np.uint32)[0])
        assert n <= cap
        return [int(x) for x in cuts.cpu().numpy()[:n]]

    def _inflate(self, fn, s, wrap, cuts, piece_out_max, out_cap):
        import torch
        inp = self._dev(np.frombuffer(bytes(s) + b"\0" * 16, dtype=np.uint8).copy())
        cu = self._dev(np.array(cuts, dtype=np.int64))
        out = self._dev(np.full(out_cap + 256, 0x5A, dtype=np.uint8))
        w = self._dev(np.zeros(4, dtype=np.int64))       # out_len | in_used | status, detail (int32)
        p = w.data_ptr()
        self.ok(fn(self.ctx, inp.data_ptr(), len(s), wrap, cu.data_ptr(), len(cuts), piece_out_max, out.data_ptr(), out_cap, p, p + 8, p + 16,
                   p + 20, None), "inflate")
        torch.cuda.synchronize()
        words, host = w.cpu().numpy(), out.cpu().numpy()
        st, det = (int(x) for x in words[2:3].view(np.int32))
        olen = int(words[0])
        return st, det, olen, int(words[1]), bytes(host[:min(olen, out_cap)]), bool((host[out_cap:] == 0x5A).all())


@pytest.fixture(scope="module")
def ctx():
    import zmi_ctypes
    c = GpuCtx(_bind(C.CDLL(zmi_ctypes.load_product()._name)))
    yield c
    c.close()


def test_batch_decode_is_exact(engine, o, inf_selection):
    from test_gpu_parity import _inflate
    assert K.batch_exact(lambda streams, caps, wrap: _inflate(engine, streams, caps, wrap=wrap), o) > 100


def test_words_of_the_size_pass_and_the_packed_decode_are_exact(target, o, inf_selection):
    assert K.words_exact(target, o) > 100


def test_resume_is_exact(eng, inf_selection):
    assert K.resume_exact(eng) >= 10


def test_block_scan_and_block_decode_are_exact(ctx, eng, inf_selection):
    assert K.scan_exact(ctx, eng) == 3
