"""CPU tests of batch deflate / inflate against one shared preset dictionary on the emulator build (tests/emu/, -DZMI_EMU), with the
checks of tests/shared_dict_checks.py -- the ones tests/test_gpu_shared_dict.py runs on the MI355X over the whole size matrix.  The
emulator runs a workgroup's 1024 threads as fibers, and every shard hashes up to 27 KiB of dictionary: here the matrices run over
the subsets named at each test (every seam, tile and alignment case at least once); the GPU runs all of them."""
import ctypes as C

import numpy as np
import pytest

import shared_dict_checks as K
import zmi_ctypes


def _aligned(n, residue, fill):
    """n bytes at an address = residue (mod 16), with slack around them"""
    raw = np.full(n + 64, fill, dtype=np.uint8)
    at = (residue - raw.ctypes.data) % 16
    return raw, raw[at:at + n]


class EmuTarget:
    def __init__(self):
        L = zmi_ctypes.load_emu()
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.zmi_deflate_dict_bound.restype = u64
        L.zmi_deflate_dict_bound.argtypes = [u64, i32]
        L.zmi_deflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, vp, u64, vp, vp, vp]
        L.zmi_deflate_batch_shared_dict_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, vp, u32, vp, u64, vp, vp, vp]
        L.zmi_inflate_batch_shared_dict_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
        self.L = L
        self.e = zmi_ctypes.Engine(L)
        self.ctx = self.e.ctx

    def close(self):
        self.e.close()

    def bound(self, n, wrap):
        return int(self.L.zmi_deflate_bound(n, wrap))

    def dict_bound(self, n, wrap):
        return int(self.L.zmi_deflate_dict_bound(n, wrap))

    def set_scratch_limit(self, nbytes):
        assert self.L.zmi_ctx_set_scratch_limit(self.ctx, nbytes) == 0

    def _dict(self, zdict, dict_align):
        keep, d = _aligned(max(1, len(zdict or b"")), dict_align, 0x5C)
        d[:len(zdict or b"")] = np.frombuffer(zdict or b"", dtype=np.uint8)
        return keep, d

    def deflate(self, shards, level, strategy, wrap, zdict, dict_align=0, in_align=0, stride=None, max_len=None, plain=False,
                null_dict=False):
        n = len(shards)
        lens = np.array([len(s) for s in shards], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        keep_in, blob = _aligned(int(lens.sum()) + 1, in_align, 0)
        blob[:int(lens.sum())] = np.frombuffer(b"".join(shards), dtype=np.uint8)
        if max_len is None:
            max_len = int(lens.max()) if n else 0
        if stride is None:
            stride = self.bound(max_len, wrap) if plain else self.dict_bound(max_len, wrap)
        keep_out, out = _aligned(n * stride + 64, 0, 0xA5)
        olen = np.zeros(n, dtype=np.uint32)
        st = np.full(n, 77, dtype=np.int32)
        if plain:
            rc = self.L.zmi_deflate_batch_dev(self.ctx, blob.ctypes.data, off.ctypes.data, lens.ctypes.data, n, max_len, level, strategy, wrap,
                                              out.ctypes.data, stride, olen.ctypes.data, st.ctypes.data, None)
        else:
            keep_d, d = self._dict(zdict, dict_align)
            rc = self.L.zmi_deflate_batch_shared_dict_dev(self.ctx, blob.ctypes.data, off.ctypes.data, lens.ctypes.data, n, max_len, level,
                                                          strategy, wrap, None if null_dict else d.ctypes.data, len(zdict or b""),
                                                          out.ctypes.data, stride, olen.ctypes.data, st.ctypes.data, None)
        return K.collect_deflate(rc, out, stride, olen, st, n, max_len)

    def inflate(self, streams, wrap, zdict, caps, dict_align=0, gap=1):
        n = len(streams)
        lens = np.array([len(s) for s in streams], dtype=np.uint32)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(lens[:-1].astype(np.uint64))
        blob = np.frombuffer(b"".join(streams) + b"\0" * 16, dtype=np.uint8).copy()
        ooff, total = K.region_layout(caps, gap)
        keep_out, out = _aligned(total, 3, 0xEE)
        ocap = np.array(caps, dtype=np.uint32)
        olen = np.full(n, 0x7777, dtype=np.uint32)
        st = np.full(n, 77, dtype=np.int32)
        used = np.full(n, 0x7777, dtype=np.uint32)
        det = np.full(n, 77, dtype=np.int32)
        keep_d, d = self._dict(zdict, dict_align)
        rc = self.L.zmi_inflate_batch_shared_dict_dev(self.ctx, blob.ctypes.data, off.ctypes.data, lens.ctypes.data, n, wrap, d.ctypes.data,
                                                      len(zdict or b""), out.ctypes.data, ooff.ctypes.data, ocap.ctypes.data, olen.ctypes.data,
                                                      st.ctypes.data, used.ctypes.data, det.ctypes.data, None)
        return K.collect_inflate(rc, out, ooff, caps, olen, st, used, gap)


@pytest.fixture(scope="module")
def target():
    t = EmuTarget()
    yield t
    t.close()


# ---- deflate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,strategy,wrap", K.DEFLATE_CONFIGS)
def test_deflate_round_trip_matrix(target, level, strategy, wrap):
    """subset: the dictionary lengths on both sides of the 16-byte, tile and reach limits, every alignment once per length in turn;
    the 70 000-byte shard at level 1 (raw and zlib) and level 6 zlib only"""
    sub = [1, 16, 17, 1025, 27649, 40000]
    big = (level, strategy, wrap) in ((1, 0, K.RAW), (1, 0, K.ZLIB), (6, 0, K.ZLIB))
    n = 0
    for i, dl in enumerate(sub):
        k, _ = K.deflate_matrix(target, level, strategy, wrap, dict_lens=[dl], aligns=[K.DICT_ALIGNS[i % 3]], big=big and dl in (17, 40000))
        n += k
    assert n == len(sub) * len(K.SMALL_LENS) + (4 if big else 0)


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
def test_inflate_decode_matrix(target, level, wrap):
    """all dictionary lengths; one alignment per length in turn, the 70 000-byte shard at level 6 only"""
    n = 0
    for i, dl in enumerate(K.INF_DICT_LENS):
        n += K.inflate_matrix(target, level, wrap, dict_lens=[dl], aligns=[K.DICT_ALIGNS[i % 3]], big=level == 6)
    assert n == 2 * (len(K.INF_DICT_LENS) * (len(K.SMALL_LENS) + (1 if level == 6 else 0)) + 1)


def test_inflate_crafted_streams(target):
    assert K.inflate_crafted(target) == 8


def test_inflate_status_mix(target):
    assert K.inflate_status_mix(target) == 7


@pytest.mark.parametrize("wrap", [K.RAW, K.ZLIB])
def test_inflate_of_own_output(target, wrap):
    n, kept = K.deflate_matrix(target, 6, 0, wrap, dict_lens=[17, 27649], aligns=[1], big=False)
    assert K.inflate_own_output(target, kept) == n
