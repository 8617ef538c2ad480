"""Single-stream inflate of streams WITHOUT flush points on the MI355X: Engine.find_blocks (zmi_stream_find_blocks_dev, the block
scan as ordered proposals at bit positions) and Engine.inflate_plain_stream (zmi_inflate_stream_bits_dev).  Ordinary host-zlib
streams of 32 MiB in which find_cuts finds nothing, a 1.5 GiB input whose proposals lie above bit 2^32 (several scan windows and
launch groups), agreement with the marker path on the same bytes, a corrupt trailer and a proposal off by one bit."""
import zlib

import pytest

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def env():
    import torch
    from zlib_rs_amd.engine import Engine
    e = Engine(0)
    data = e.gen_shards(64, MiB)
    torch.cuda.synchronize()
    yield e, data
    e.close()


@pytest.mark.parametrize("wrap,level", [(2, 6), (1, 9)])
def test_ordinary_stream(env, wrap, level):
    import numpy as np
    import torch
    e, data = env
    host = bytes(data[:32 * MiB].cpu().numpy())
    c = zlib.compressobj(level, zlib.DEFLATED, {1: 15, 2: 31}[wrap])
    s = c.compress(host) + c.flush()
    dev = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(e.device)
    assert e.find_cuts(dev, wrap=wrap, min_gap=1).numel() == 1      # no flush point: the marker path has one piece
    cuts = e.find_blocks(dev, wrap=wrap, min_gap=1 << 15)
    assert cuts.numel() > 100
    c = cuts.tolist()
    assert c[0] == 8 * {1: 2, 2: 10}[wrap] and all(b >= a + (8 << 15) for a, b in zip(c, c[1:]))
    assert torch.equal(e.find_blocks(dev, wrap=wrap, min_gap=1 << 15), cuts)
    back, used = e.inflate_plain_stream(dev, wrap=wrap, min_gap=1 << 15)
    assert used == len(s) and torch.equal(back, data[:32 * MiB])


def test_positions_above_2_pow_32_bits(env):
    """more than 512 MiB of compressed bytes: eleven scan windows, 64-bit positions, several launch groups"""
    import torch
    e, _ = env
    n_mib = 1536
    big = e.gen_shards(n_mib, MiB)
    s = e.deflate_stream(big, level=6, wrap=2).clone()
    assert s.numel() > 512 * MiB
    cuts = e.find_blocks(s, wrap=2)
    c = cuts.tolist()
    assert c[-1] > 1 << 32 and all(b >= a + (8 << 16) for a, b in zip(c, c[1:]))
    back, used = e.inflate_plain_stream(s, wrap=2, bit_index=cuts, out_cap=n_mib * MiB)
    assert used == s.numel() and back.numel() == n_mib * MiB and torch.equal(back, big)
    del big, back, s, cuts
    torch.cuda.empty_cache()


def test_marker_path_and_block_path_agree(env):
    import torch
    e, data = env
    s, idx = e.deflate_stream(data, level=6, wrap=2, piece_bytes=MiB, index=True)
    a, used_a = e.inflate_stream(s, wrap=2, index=idx[:-1], piece_out_max=MiB)
    b, used_b = e.inflate_plain_stream(s, wrap=2)
    assert used_a == used_b == s.numel() and torch.equal(a, b) and torch.equal(a, data)


def test_errors_and_recovery(env):
    from zlib_rs_amd import _lib
    import torch
    e, data = env
    part = data[:32 * MiB]
    s = e.deflate_stream(part, level=6, wrap=2, piece_bytes=MiB)
    bad = s.clone()
    bad[-6] ^= 1                                       # CRC-32
    with pytest.raises(RuntimeError, match="status -3"):
        e.inflate_plain_stream(bad, wrap=2)
    cuts = e.find_blocks(s, wrap=2).clone()
    assert cuts.numel() > 20
    cuts[5] += 1
    meta = torch.zeros(3, dtype=torch.int64, device=e.device)
    out = torch.empty(part.numel(), dtype=torch.uint8, device=e.device)
    _lib.check(e.L.zmi_inflate_stream_bits_dev(e._ctx, s.data_ptr(), s.numel(), 2, cuts.data_ptr(), cuts.numel(), MiB, out.data_ptr(), out.numel(),
                                               meta.data_ptr(), meta.data_ptr() + 8, meta.data_ptr() + 16, meta.data_ptr() + 20, None),
               "inflate_stream_bits")
    torch.cuda.synchronize()
    sd = meta.tolist()[2]
    st, det = sd & 0xFFFFFFFF, (sd >> 32) & 0xFFFFFFFF
    assert st != 0 and det & 0xFF == 3 and det >> 8 == 5
    # the Python layer drops the cut that did not verify and runs again
    back, used = e.inflate_plain_stream(s, wrap=2, bit_index=cuts)
    assert torch.equal(back, part) and used == s.numel()
