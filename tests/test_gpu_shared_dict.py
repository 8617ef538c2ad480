"""GPU tests (-m gpu) of batch deflate / inflate against one shared preset dictionary through zlib_rs_amd.engine.Engine
(deflate_batch / inflate_batch with zdict=...), with the checks of tests/shared_dict_checks.py over the whole size matrix.  Here the
kernels run as they ship: the dictionary instantiations of the match search (csrc/lz77.hip) and of the one-wave-per-stream resolve
pass (csrc/inflate.hip), the DICTID through the checksum kernel's byte sums.  Every launch is a few MB at most."""
import numpy as np
import pytest

import shared_dict_checks as K

pytestmark = pytest.mark.gpu


class GpuTarget:
    def __init__(self, engine):
        import torch
        from zlib_rs_amd import _lib
        self.torch, self.e, self.lib = torch, engine, _lib

    def _at(self, data, residue, pad=64):
        """the bytes on the device at an address = residue (mod 16) (allocations are 256-byte aligned)"""
        t = self.torch.zeros(len(data) + residue + pad, dtype=self.torch.uint8, device=self.e.device)
        if len(data):
            t[residue:residue + len(data)] = self.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.e.device)
        v = t[residue:residue + len(data)]
        assert v.data_ptr() % 16 == residue
        return v

    def _i64(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(self.e.device)

    def _i32(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.e.device)

    def bound(self, n, wrap):
        return self.e.deflate_bound(n, wrap)

    def dict_bound(self, n, wrap):
        return self.e.deflate_bound(n, wrap, zdict=True)

    def set_scratch_limit(self, nbytes):
        self.lib.check(self.e.L.zmi_ctx_set_scratch_limit(self.e._ctx, int(nbytes)), "zmi_ctx_set_scratch_limit")

    def deflate(self, shards, level, strategy, wrap, zdict, dict_align=0, in_align=0, stride=None, max_len=None, plain=False,
                null_dict=False):
        torch, n = self.torch, len(shards)
        lens = np.array([len(s) for s in shards], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        blob = self._at(b"".join(shards), in_align)
        if max_len is None:
            max_len = int(lens.max()) if n else 0
        if stride is None:
            stride = self.bound(max_len, wrap) if plain else self.dict_bound(max_len, wrap)
        out = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device=self.e.device)
        olen = torch.zeros(n, dtype=torch.int32, device=self.e.device)
        st = torch.full((n,), 77, dtype=torch.int32, device=self.e.device)
        d_off, d_len = self._i64(off), self._i32(lens)
        try:
            if plain:
                self.e.deflate_batch(blob, d_off, d_len, max_len, level=level, strategy=strategy, wrap=wrap, out=out[:n * stride].view(n, stride),
                                     out_len=olen, status=st)
            elif null_dict:   # (the engine passes NULL for an empty tensor only: d_dict = NULL with a length goes to the library directly)
                self.lib.check(self.e.L.zmi_deflate_batch_shared_dict_dev(self.e._ctx, blob.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, max_len,
                                                                          level, strategy, wrap, None, len(zdict), out.data_ptr(), stride,
                                                                          olen.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream),
                               "zmi_deflate_batch_shared_dict_dev")
            else:
                self.e.deflate_batch(blob, d_off, d_len, max_len, level=level, strategy=strategy, wrap=wrap, out=out[:n * stride].view(n, stride),
                                     out_len=olen, status=st, zdict=self._at(zdict or b"", dict_align))
        except RuntimeError as err:
            return int(str(err).split("rc=")[1].split()[0]), [], [], False
        return K.collect_deflate(0, out.cpu().numpy(), stride, olen.cpu().numpy().view(np.uint32), st.cpu().numpy(), n, max_len)

    def inflate(self, streams, wrap, zdict, caps, dict_align=0, gap=1):
        torch, n = self.torch, len(streams)
        lens = np.array([len(s) for s in streams], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        blob = self._at(b"".join(streams), 0)
        ooff, total = K.region_layout(caps, gap)
        whole = torch.full((total + 16,), 0xEE, dtype=torch.uint8, device=self.e.device)
        out = whole[3:3 + total]          # the regions start at an odd address
        olen = torch.full((n,), 0x7777, dtype=torch.int32, device=self.e.device)
        st = torch.full((n,), 77, dtype=torch.int32, device=self.e.device)
        used = torch.full((n,), 0x7777, dtype=torch.int32, device=self.e.device)
        det = torch.full((n,), 77, dtype=torch.int32, device=self.e.device)
        try:
            self.e.inflate_batch(blob, self._i64(off), self._i32(lens), out, self._i64(ooff), self._i32(caps), wrap=wrap, out_len=olen, status=st,
                                 zdict=self._at(zdict or b"", dict_align), in_used=used, detail=det)
        except RuntimeError as err:
            return int(str(err).split("rc=")[1].split()[0]), [], [], [], [], False
        return K.collect_inflate(0, out.cpu().numpy(), ooff, caps, olen.cpu().numpy().view(np.uint32), st.cpu().numpy(),
                                 used.cpu().numpy().view(np.uint32), gap)


@pytest.fixture(scope="module")
def target(engine):
    return GpuTarget(engine)


_KEPT = {}


# ---- deflate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,strategy,wrap", K.DEFLATE_CONFIGS)
def test_deflate_round_trip_matrix(target, level, strategy, wrap):
    """14 dictionary lengths x 3 alignments x 10 shard lengths, and the 70 000-byte shard once per dictionary length"""
    n, kept = K.deflate_matrix(target, level, strategy, wrap)
    assert n == len(K.DICT_LENS) * (3 * len(K.SMALL_LENS) + 2)
    if (level, strategy) == (6, 0):
        _KEPT[wrap] = kept


def test_deflate_seam(target):
    assert K.deflate_seam(target) == 6


def test_deflate_uses_the_dictionary(target):
    assert K.deflate_uses_dictionary(target) == 5


@pytest.mark.parametrize("level", [6, 9])
def test_ratio_on_text(target, level):
    excess, ours, without, ref = K.deflate_ratio(target, level)
    print("level %d: %d bytes with the dictionary, %d without, zlib %d: excess %.2f %%" % (level, ours, without, ref, excess))
    assert ours < without
    assert excess <= K.RATIO_EXCESS_MEASURED[level] + K.RATIO_SLACK


def test_deflate_exact_equalities(target):
    assert K.deflate_equalities(target) == 10


def test_deflate_arguments(target):
    assert K.deflate_arguments(target) == 4


# ---- inflate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB])
@pytest.mark.parametrize("level", [1, 6, 9])
def test_inflate_decode_matrix(target, inf_selection, level, wrap):
    assert K.inflate_matrix(target, level, wrap) == 2 * (len(K.INF_DICT_LENS) * (3 * len(K.SMALL_LENS) + 1) + 3)


def test_inflate_crafted_streams(target, inf_selection):
    assert K.inflate_crafted(target) == 8


def test_inflate_status_mix(target, inf_selection):
    assert K.inflate_status_mix(target) == 7


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB])
def test_inflate_of_own_output(target, inf_selection, wrap):
    """the level 6 streams of the round-trip matrix (made again when that test did not run in this process)"""
    if wrap not in _KEPT:
        _KEPT[wrap] = K.deflate_matrix(target, 6, 0, wrap)[1]
    kept = _KEPT[wrap]
    assert K.inflate_own_output(target, kept) == sum(len(k[2]) for k in kept)
