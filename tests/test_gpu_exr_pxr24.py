"""OpenEXR PXR24 (compression 5) on the MI355X: the checks of tests/exr_pxr24_checks.py over their whole matrices through the library's C
ABI on torch buffers -- the reader under both decode-kernel selections --, the writer under a scratch limit that forces several launch
groups, then the Engine layer (exr_headers / exr_read of a crafted file, save_exr(compression="pxr24")) and a frame of real size."""
import os

import numpy as np
import pytest
import torch

import exr_pxr24_checks as K
import png_write_checks as PW
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


def _set_group(pieces):
    if pieces:
        os.environ["ZMI_STREAM_GROUP"] = str(pieces)
    else:
        os.environ.pop("ZMI_STREAM_GROUP", None)


def test_read_geometry(target, inf_selection):
    """widths 1, 2, 3, 5, 63, 64, 65, T - 1, T, T + 1 and 2 T + 1 x heights 1, 15, 16, 17 and 33 x one HALF channel, RGBA HALF, G HALF +
    Z FLOAT + id UINT, FLOAT alone, UINT alone"""
    assert K.read_geometry(target) == 5 * 11 * 5


def test_read_tiles(target, inf_selection):
    assert K.read_tiles(target) == 10


def test_read_values(target, inf_selection):
    assert K.read_values(target) == 12


def test_read_raw_chunks(target, inf_selection):
    assert K.read_raw_chunks(target) == 4


def test_read_faults(target, inf_selection):
    assert K.read_faults(target) == 7


def test_read_independence(target, inf_selection):
    assert K.read_independence(target) == 4 + 2 + 6


@pytest.mark.parametrize("layout", range(5), ids=["one HALF channel", "RGBA HALF", "G HALF + Z FLOAT + id UINT", "FLOAT alone", "UINT alone"])
def test_write_geometry(target, layout):
    assert K.write_geometry(target, layouts=K.LAYOUTS[layout:layout + 1]) == 11 * 5


def test_write_tiles(target):
    assert K.write_tiles(target) == 4


def test_write_values(target):
    assert K.write_values(target) == 11


def test_write_raw_rule(target):
    assert K.write_raw_rule(target) == 4


def test_write_pieces_and_launch_groups(target):
    assert K.write_pieces(target, set_group=_set_group) == 16 + 2


def test_write_independence(target):
    assert K.write_independence(target) == 5


def test_write_launch_groups_under_the_smallest_scratch_limit(target):
    """16 tiles of 512 x 512 of G HALF + Z FLOAT (m = 1.25 MiB: two pieces of 1 MiB each) under the smallest scratch limit, 64 MiB: a
    group holds at most 12 pieces = 6 chunks, so the 16 chunks need three groups.  Level 1 keeps it in seconds; the bytes must be those
    of the one group the default limit gives"""
    p = K.craft(2048, 2048, (("G", K.HALF), ("Z", K.FLOAT)), tile=(512, 512), noise=(5,), seed=21, level=1)
    per_piece = PW.launch_group(target, 64 << 20, 1 << 20, 1 << 20)
    assert 2 <= per_piece < 32 and PW.launch_group(target, 8 << 30, 1 << 20, 1 << 20) >= 32
    src = [K.source(p)]
    ref = target.write(src, pb=1 << 20, level=1, align=16)
    K.write_check(target, ref, [p], pb=1 << 20, level=1, align=16, exact=False)
    assert target.L.zmi_ctx_set_scratch_limit(target.ctx, 64 << 20) == 0
    try:
        r = target.write(src, pb=1 << 20, level=1, align=16)
    finally:
        assert target.L.zmi_ctx_set_scratch_limit(target.ctx, 8 << 30) == 0
    assert (r.rc, r.off, r.len, r.status, r.guard_ok) == (0, ref.off, ref.len, ref.status, True) and r.out == ref.out


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _dev(e, plane):
    dt = {"<f2": torch.float16, "<f4": torch.float32, "<u4": torch.int32}[plane.dtype.str]
    return torch.from_numpy(plane.view(np.uint8).copy()).to(e.device).view(dt).view(plane.shape)


def test_engine_reads_a_crafted_file(target):
    e = target.e
    files = [K.craft(21, 40, K.MIXED, xmin=-3, ymin=7, seed=1), K.craft(40, 33, K.ONE_FLOAT, tile=(16, 16), order=2, seed=3, noise=(4,))]
    b = e.exr_headers([p.blob for p in files])
    assert [b.status(i) for i in range(2)] == [0, 0] and b.readable == [True, True]
    assert [b.record(i)["lines_per_chunk"] for i in range(2)] == [16, 16] and [b.record(i)["compression"] for i in range(2)] == [5, 5]
    out, off, ln, st = e.exr_read(b)
    assert st.tolist() == [0, 0] and e.last_exr_detail.tolist() == [0, 0]
    for j, p in enumerate(files):
        got, want = _host(out[int(off[j]):int(off[j]) + int(ln[j])]), p.want
        assert len(got) == len(want) and all(got[a:a + n] == want[a:a + n] for a, n in _planes(p)), j


def _planes(p):
    """(offset, bytes) of every plane of the region: the bytes between them belong to nobody"""
    return [(o, p.width * p.height * K.SIZE[t]) for o, (_, t) in zip(p.plane_off, p.channels)]


def test_engine_save_exr_is_read_by_the_reference_reader(target):
    e = target.e
    p = K.craft(37, 21, K.MIXED, seed=4, xmin=-5, ymin=3)
    image = {"id": _dev(e, p.planes[2]), "Z": _dev(e, p.planes[1]), "G": _dev(e, p.planes[0])}
    blob = e.save_exr(image, compression="pxr24", origin=(-5, 3), piece_bytes=512, align=1)
    assert blob == K.expected(target, p, 512, 6, 0).blob
    region, stored = K.read_file(blob, p)
    assert stored == [False, False] and region == K.lossy_region(p, stored)
    assert e.last_exr_chunk_len.tolist() == [[s for s, _ in K.W.chunks(blob, p)]]
    assert int(e.exr_bound((21, 37), [("G", torch.float16), ("Z", torch.float32), ("id", torch.int32)], compression="pxr24")) >= len(blob)
    b = e.exr_headers(blob)
    back, boff, _, bst = e.exr_read(b)
    assert bst.tolist() == [0] and b.record(0)["compression"] == 5
    lossy = K.f24_fast(p.planes[1].view("<u4")) << np.uint32(8)
    assert _host(b.channel(back, boff, 0, "Z")) == lossy.tobytes() and _host(b.channel(back, boff, 0, "G")) == p.planes[0].tobytes()
    assert _host(b.channel(back, boff, 0, "id")) == p.planes[2].tobytes()
    with pytest.raises(ValueError):
        e.save_exr(image, compression="piz")


@pytest.mark.parametrize("kind", ["one frame of 2048 x 1080 RGBA HALF", "1021 x 515 FLOAT in tiles of 256 x 256 at level 1"])
def test_frames_of_real_size(target, kind):
    if kind.startswith("one frame"):
        p, level = K.craft(2048, 1080, K.RGBA, noise=(9,), seed=6, level=1), 6
    else:
        p, level = K.craft(1021, 515, K.ONE_FLOAT, tile=(256, 256), xmin=-11, ymin=40, seed=7, level=1), 1
    b, r = K.X.run(target.reader, [p], align=16)
    w = target.write([K.source(p)], pb=1 << 20, level=level, align=16)
    stored = K.write_check(target, w, [p], pb=1 << 20, level=level, align=16, exact=False)
    assert sum(stored[0]) == (1 if kind.startswith("one frame") else 0)
