"""The TIFF reader on the MI355X: the checks of tests/tiff_checks.py over their whole matrices through the library's C ABI on torch
buffers, then the Engine layer (tiff_directory, TiffFile, tiff_read in both modes), both decode-kernel selections, and two images of
the sizes real files have."""
import numpy as np
import pytest
import torch

import tiff_checks as K
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


def test_geometry(target):
    """tiles of 16 x 16 and 16 x 32 at k * tile, k * tile +- 1, 1 x 1 and one tile; the strip cases; row bytes at the row tile - 1, + 0,
    + 1 and 2 x + 1 in pixels of 1, 3, 4, 6 and 8 bytes"""
    assert K.geometry(target) == 2 * 5 + 9 + 5 * 4


def test_formats(target):
    assert K.formats(target) == 88 + 5


def test_layout(target):
    assert K.layout(target) == 12 + 4 + 1 + 1


def test_selection_and_room(target):
    assert K.selection(target) == 4 * 16 + 3 + 3 + 2 + 2


def test_statuses(target):
    assert K.statuses(target) == 10 + 24 + 6


def test_forged_record(target):
    assert K.forged_record(target) == 14


def test_determinism(target, inf_selection):
    assert K.determinism(target) == 7


def test_arguments(target):
    assert K.arguments(target) == 14


# ---- the Engine layer ---------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def test_engine_directory_and_both_modes(target):
    e = target.e
    pages = [K.Page(50, 40, 3, 8, pred=2, tile=(16, 16), seed=1, sparse=(5,)), K.Page(33, 20, 1, 32, 3, 3, rps=3, seed=2),
             K.Page(9, 7, 2, 16, 2, 2, rps=4, comp=1, seed=3), K.Page(20, 20, 3, 8, pred=2, tile=(16, 16), seed=4, tags={259: (K.SHORT, [5])})]
    blob = K.Tiff(pages, be=True).blob
    tf = e.tiff_directory(blob)
    assert tf.n_pages == 4 and tf.info["n_pages"] == 4 and tf.info["big_endian"] == 1 and tf.info["bigtiff"] == 0
    assert tf.status.tolist() == [0, 0, 0, K.TP_COMPRESSION] and tf.readable.tolist() == [True, True, True, False]
    assert [tf.shape(p) for p in range(3)] == [(40, 50, 3), (20, 33, 1), (7, 9, 2)]
    assert [tf.dtype(p) for p in range(3)] == [torch.uint8, torch.float32, torch.int16]
    assert tf.tile_shape(0) == (16, 16, 3) and tf.grid(0) == (3, 4) and tf.tile_shape(1) == (3, 33, 1) and tf.grid(1) == (7, 1)
    for p in range(3):
        img, st = e.tiff_read(None, tf, page=p)
        assert tuple(img.shape) == tf.shape(p) and img.dtype == tf.dtype(p) and _host(img) == pages[p].image
        assert st.tolist() == [0] * pages[p].n_segs
    assert e.last_tiff_detail.tolist() == [0, 0]
    img, st = e.tiff_read(None, tf, page=0)
    assert e.last_tiff_detail.tolist() == [0] * 5 + [K.TE_SPARSE] + [0] * 6
    # a selection assembled into a zeroed image; the same into a caller's buffer, which keeps what no segment covers
    img, st = e.tiff_read(None, tf, page=0, segments=[6, 1])
    want = np.zeros((40, 50, 3), dtype=np.uint8)
    full = np.frombuffer(pages[0].image, dtype=np.uint8).reshape(40, 50, 3)
    want[16:32, 32:48], want[0:16, 16:32] = full[16:32, 32:48], full[0:16, 16:32]
    assert st.tolist() == [0, 0] and _host(img) == want.tobytes()
    buf = torch.full((40 * 50 * 3 + 7,), K.FILL, dtype=torch.uint8, device=e.device)
    img, st = e.tiff_read(None, tf, page=0, segments=torch.tensor([6, 1], dtype=torch.int32, device=e.device), out=buf)
    want2 = np.full((40, 50, 3), K.FILL, dtype=np.uint8)
    want2[16:32, 32:48], want2[0:16, 16:32] = full[16:32, 32:48], full[0:16, 16:32]
    assert img.data_ptr() == buf.data_ptr() and _host(img) == want2.tobytes() and _host(buf[-7:]) == bytes([K.FILL]) * 7
    # dense: whole tiles with their padding, out_off at multiples of align, views as they stand
    out, off, ln, st = e.tiff_read(None, tf, page=0, segments=[11, 0, 40], assemble=False)
    assert st.tolist() == [0, 0, K.E_ARG] and ln.tolist() == [768, 768, 0] and off.tolist() == [0, 768, 1536, 1536]
    assert _host(out[:768]) == pages[0].segs[11] and _host(out[768:1536]) == pages[0].segs[0]
    out, off, ln, st = e.tiff_read(None, tf, page=1, assemble=False, align=4096)
    assert st.tolist() == [0] * 7 and off.tolist()[:7] == [4096 * j for j in range(7)] and ln.tolist() == [396] * 6 + [264]
    strip = out[4096 * 6:4096 * 6 + 264].view(torch.float32).view(2, 33, 1)
    assert _host(strip) == pages[1].segs[6]
    # a flagged page, a page behind the table, bytes in one call
    img, st = e.tiff_read(None, tf, page=3)
    assert img.numel() == 0 and st.tolist() == [K.Z_VERSION_ERROR] and e.last_tiff_detail.tolist() == [K.TP_COMPRESSION]
    img, st = e.tiff_read(None, tf, page=9)
    assert img.numel() == 0 and st.tolist() == [K.E_ARG]
    img, st = e.tiff_read(K.Tiff([pages[2]], big=True).blob)
    assert _host(img) == pages[2].image
    with pytest.raises(RuntimeError, match="case 1"):
        e.tiff_directory(b"II" + bytes(30))
    many = K.Tiff([K.Page(3, 3, 1, 8, seed=k) for k in range(70)])
    assert e.tiff_directory(many.blob).n_pages == 70 and e.tiff_directory(many.blob, cap=5).n_pages == 5


@pytest.mark.parametrize("kind", ["rgb8 predictor 2, 8 x 8 tiles of 256 x 256", "float32 predictor 3, 4 x 4 tiles of 512 x 512"])
def test_engine_images_of_real_sizes(target, kind):
    e = target.e
    if kind.startswith("rgb8"):
        p = K.Page(2048 - 37, 2048 - 5, 3, 8, pred=2, tile=(256, 256), seed=5, level=1)
    else:
        p = K.Page(2048 - 37, 2048 - 5, 1, 32, 3, 3, tile=(512, 512), seed=6, level=1)
    tf = e.tiff_directory(K.Tiff([p], big=True).blob)
    img, st = e.tiff_read(None, tf)
    assert st.tolist() == [0] * p.n_segs and tuple(img.shape) == (p.height, p.width, p.samples)
    assert _host(img) == p.image
    out, off, ln, st = e.tiff_read(None, tf, segments=[p.n_segs - 1, 0], assemble=False)
    assert st.tolist() == [0, 0] and _host(out[:int(ln[0])]) == p.segs[-1] and _host(out[int(off[1]):int(off[1]) + int(ln[1])]) == p.segs[0]
