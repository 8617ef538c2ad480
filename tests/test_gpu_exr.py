"""The OpenEXR reader on the MI355X: the checks of tests/exr_checks.py over their whole matrices through the library's C ABI on torch
buffers, both decode-kernel selections, then the Engine layer (exr_headers, ExrBatch, exr_read) and images of the sizes real files have."""
import numpy as np
import pytest
import torch

import exr_checks as K
from test_gpu_zip import TorchMem

pytestmark = pytest.mark.gpu


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


def test_geometry(target, inf_selection):
    """widths 1, 2, 3, 5, 17, 63, 64, 65 and 257 x heights 1, 15, 16, 17 and 33 x ZIPS, ZIP, NONE x one HALF channel, RGBA HALF, G HALF +
    Z FLOAT + id UINT"""
    assert K.geometry(target) == 3 * 3 * 9 * 5


def test_trips(target, inf_selection):
    assert K.trips(target) == 20


def test_carries(target, inf_selection):
    assert K.carries(target) == 1


def test_raw_chunks(target, inf_selection):
    assert K.raw_chunks(target) == 4


def test_tiles(target, inf_selection):
    assert K.tiles(target) == 12


def test_layout(target, inf_selection):
    assert K.layout(target) == 22


def test_statuses(target, inf_selection):
    assert K.statuses(target) == 40 + 26


def test_selection_and_room(target, inf_selection):
    assert K.selection(target) == 10 + 4 + 5


def test_forged_record(target, inf_selection):
    assert K.forged_record(target) == 24


def test_independence(target, inf_selection):
    assert K.independence(target) == 9


def test_arguments(target):
    assert K.arguments(target) == 11


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def test_engine_headers_batch_and_read(target):
    e = target.e
    files = [K.Exr(21, 40, K.RGBA, K.ZIP, xmin=-3, ymin=7, seed=1), K.Exr(33, 20, K.MIXED, K.ZIPS, seed=2),
             K.Exr(40, 33, K.MIXED, K.ZIP, tile=(16, 16), order=2, seed=3), [p for n, p in K.header_faults() if n == "compression 4"][0],
             K.Exr(9, 7, K.ONE_HALF, K.NONE, seed=4)]
    b = e.exr_headers([p.blob for p in files])
    assert b.n == 5 and [b.status(i) for i in range(5)] == [0, 0, 0, K.XE_COMPRESSION, 0] and b.readable == [True, True, True, False, True]
    assert [b.shape(i) for i in range(5)] == [(4, 40, 21), (3, 20, 33), (3, 33, 40), (3, 20, 10), (1, 7, 9)]
    assert b.channels(0) == [(n, torch.float16) for n in "ABGR"]
    assert b.channels(1) == [("G", torch.float16), ("Z", torch.float32), ("id", torch.int32)]
    assert b.windows(0) == ((-3, 7, 17, 46), (0, 0, 20, 39)) and b.tiled(0) is None and b.tiled(2) == (16, 16)
    assert b.record(2)["n_chunks"] == 9 and b.record(0)["lines_per_chunk"] == 16
    out, off, ln, st = e.exr_read(b)
    assert st.tolist() == [0, 0, 0, K.Z_VERSION_ERROR, 0] and e.last_exr_detail.tolist() == [0, 0, 0, K.XE_COMPRESSION, 0]
    assert int(off[-1]) == out.numel() and ln.tolist() == [p.region_bytes if not p.flag else 0 for p in files]
    img = b.image(out, off, 0)
    assert tuple(img.shape) == (4, 40, 21) and img.dtype == torch.float16
    assert _host(img) == b"".join(p.tobytes() for p in files[0].planes)
    with pytest.raises(ValueError, match="differ"):
        b.image(out, off, 1)
    for j in (1, 2):
        for c, (name, dt) in enumerate(b.channels(j)):
            ch = b.channel(out, off, j, name)
            assert ch.dtype == dt and tuple(ch.shape) == b.shape(j)[1:] and _host(ch) == files[j].planes[c].tobytes(), (j, name)
    assert torch.equal(b.channel(out, off, 1, "Z"), torch.from_numpy(files[1].planes[1].astype(np.float32)).to(e.device))
    with pytest.raises(KeyError):
        b.channel(out, off, 0, "Z")
    # a selection with a duplicate and a bad index, a list of device tensors, one file as bytes, a caller's buffer one byte short
    out2, off2, ln2, st2 = e.exr_read(b, sel=[4, 0, 9, 4], align=64)
    assert st2.tolist() == [0, 0, K.E_ARG, 0] and off2.tolist()[:2] == [0, 128]
    assert _host(b.image(out2, off2, 1, file=0)) == _host(img) and _host(b.image(out2, off2, 3, file=4)) == files[4].planes[0].tobytes()
    tens = [torch.from_numpy(np.frombuffer(p.blob, dtype=np.uint8).copy()).to(e.device) for p in files[:2]]
    b2 = e.exr_headers(tens)
    o, f, _, s = e.exr_read(b2, sel=torch.tensor([1], dtype=torch.int32, device=e.device))
    assert s.tolist() == [0] and b2.channels(1)[1] == ("Z", torch.float32) and _host(b2.channel(o, f, 0, "id", file=1)) == files[1].planes[2].tobytes()
    b3 = e.exr_headers(files[2].blob)
    o, f, _, s = e.exr_read(b3)
    assert s.tolist() == [0] and _host(b3.channel(o, f, 0, "G")) == files[2].planes[0].tobytes()
    short = torch.full((files[4].region_bytes - 1,), 7, dtype=torch.uint8, device=e.device)
    o, f, l, s = e.exr_read(b, sel=[4], out=short)
    assert s.tolist() == [K.Z_BUF_ERROR] and e.last_exr_detail.tolist() == [K.XE_OUT] and l.tolist() == [0] and bool((short == 7).all())
    many = K.Exr(4, 4, tuple(("c%02d" % k, K.HALF) for k in range(40)), K.ZIP, seed=3)
    assert e.exr_headers(many.blob).status(0) == K.XE_CHANNELS and e.exr_headers(many.blob, chan_cap=40).status(0) == 0


def test_engine_image_of_half_planes_with_padding_between_them(target):
    """several HALF channels of an odd W * H: the planes stand 2 bytes apart, image() is a strided view over them, channel() dense"""
    e = target.e
    files = [K.Exr(3, 3, K.RGBA[1:], K.ZIP, seed=1), K.Exr(1, 1, K.RGBA, K.ZIPS, seed=2), K.Exr(33, 17, K.RGBA, K.ZIP, seed=3),
             K.Exr(5, 7, (("Y", K.FLOAT), ("Z", K.FLOAT)), K.ZIP, seed=4)]
    b = e.exr_headers([p.blob for p in files])
    assert [b.record(i)["region_bytes"] for i in range(4)] == [58, 14, 4 * 33 * 17 * 2 + 6, 280]
    out, off, ln, st = e.exr_read(b)
    assert st.tolist() == [0] * 4 and ln.tolist() == [58, 14, 4 * 33 * 17 * 2 + 6, 280]
    for j, p in enumerate(files):
        img = b.image(out, off, j)
        c, h, w = b.shape(j)
        assert tuple(img.shape) == (c, h, w) and img.data_ptr() == out.data_ptr() + int(off[j])
        assert img.is_contiguous() == (j == 3) and img.stride()[0] == (h * w + 1 if j < 3 else h * w)
        assert _host(img) == b"".join(x.tobytes() for x in p.planes), j
        for k, (name, _) in enumerate(b.channels(j)):
            assert torch.equal(b.channel(out, off, j, name), img[k]), (j, name)


@pytest.mark.parametrize("kind", ["two frames of 512 x 512 RGBA HALF, ZIP", "1024 x 256 FLOAT in tiles of 64 x 64"])
def test_engine_images_of_real_sizes(target, kind):
    e = target.e
    if kind.startswith("two"):
        files = [K.Exr(512, 512, K.RGBA, K.ZIP, seed=5, level=1, noise=(7,)), K.Exr(512, 512, K.RGBA, K.ZIP, seed=6, level=1, order=1)]
    else:
        files = [K.Exr(1024, 256, (("Z", K.FLOAT),), K.ZIP, tile=(64, 64), order=2, seed=7, level=1)]
    b = e.exr_headers([p.blob for p in files])
    out, off, ln, st = e.exr_read(b)
    assert st.tolist() == [0] * len(files)
    for j, p in enumerate(files):
        assert _host(out[int(off[j]):int(off[j]) + int(ln[j])]) == p.want
        assert _host(b.image(out, off, j)) == b"".join(x.tobytes() for x in p.planes)
