"""Single-stream inflate on the MI355X: Engine.inflate_stream / zmi_inflate_stream_dev on this library's own streams (256 MiB, every
wrap and mode; the 4 GiB + 3 MiB gzip stream of test_stream_above_4gib, decoded on the device under the default scratch limit), a
64 MiB pigz-shaped stream of Python's zlib read through find_cuts, a corrupt trailer and a wrong index."""
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def env():
    import torch
    from zlib_rs_amd.engine import Engine
    e = Engine(0)
    data = e.gen_shards(256, MiB)
    torch.cuda.synchronize()
    yield e, data
    e.close()


def test_256mib_per_wrap_and_mode(env):
    import torch
    e, data = env
    for wrap in (0, 1, 2):
        for independent in (False, True):
            s, idx = e.deflate_stream(data, level=6, wrap=wrap, piece_bytes=MiB, independent=independent, index=True)
            back, used = e.inflate_stream(s, wrap=wrap, index=idx[:-1], piece_out_max=MiB)
            assert used == s.numel() and torch.equal(back, data), (wrap, independent)


def test_stream_above_4gib_on_device(env):
    """4 GiB + 3 MiB of gzip: ISIZE wraps, several launch groups under the default scratch limit"""
    import torch
    e, _ = env
    n_mib = 4096 + 3
    big = e.gen_shards(n_mib, MiB)
    s, idx = e.deflate_stream(big, level=6, wrap=2, index=True)
    assert int.from_bytes(s[-4:].cpu().numpy().tobytes(), "little") == (n_mib * MiB) % (1 << 32)
    back, used = e.inflate_stream(s, wrap=2, index=idx[:-1], piece_out_max=MiB, out_cap=n_mib * MiB)
    assert used == s.numel() and back.numel() == n_mib * MiB and torch.equal(back, big)
    del big, back, s, idx
    torch.cuda.empty_cache()


def test_pigz_shaped_stream_through_find_cuts(env):
    import numpy as np
    import torch
    e, data = env
    host = bytes(data[:64 * MiB].cpu().numpy())
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    parts = []
    for lo in range(0, len(host), 128 << 10):
        parts.append(c.compress(host[lo:lo + (128 << 10)]))
        parts.append(c.flush(zlib.Z_SYNC_FLUSH))
    parts.append(c.flush())
    s = b"".join(parts)
    want = zlib.decompress(s, 31)
    dev = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(e.device)
    cuts = e.find_cuts(dev, wrap=2, min_gap=64 << 10)
    assert cuts.numel() > 256
    back, used = e.inflate_stream(dev, wrap=2, index=cuts, piece_out_max=128 << 10)
    assert used == len(s) and bytes(back.cpu().numpy()) == want


def test_corrupt_trailer_and_wrong_index(env):
    from zlib_rs_amd import _lib
    import torch
    e, data = env
    part = data[:32 * MiB]
    s, idx = e.deflate_stream(part, level=6, wrap=2, piece_bytes=MiB, index=True)
    bad = s.clone()
    bad[-6] ^= 1                                       # CRC-32
    with pytest.raises(RuntimeError, match="status -3"):
        e.inflate_stream(bad, wrap=2, index=idx[:-1], piece_out_max=MiB)
    cuts = idx[:-1].clone()
    cuts[5] += 1
    meta = torch.zeros(3, dtype=torch.int64, device=e.device)
    out = torch.empty(part.numel(), dtype=torch.uint8, device=e.device)
    _lib.check(e.L.zmi_inflate_stream_dev(e._ctx, s.data_ptr(), s.numel(), 2, cuts.data_ptr(), cuts.numel(), MiB, out.data_ptr(), out.numel(),
                                          meta.data_ptr(), meta.data_ptr() + 8, meta.data_ptr() + 16, meta.data_ptr() + 20, None), "inflate_stream")
    torch.cuda.synchronize()
    sd = meta.tolist()[2]
    st, det = sd & 0xFFFFFFFF, (sd >> 32) & 0xFFFFFFFF
    assert st != 0 and det & 0xFF == 3
    # the Python layer drops the cut that did not verify and runs again
    back, used = e.inflate_stream(s, wrap=2, index=cuts, piece_out_max=MiB)
    assert torch.equal(back, part) and used == s.numel()
