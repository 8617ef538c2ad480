"""The TIFF writer on the MI355X: the checks of tests/tiff_write_checks.py over their whole matrices through the library's C ABI on torch
buffers, then the Engine layer (tiff_bound, tiff_write in both input forms, save_tiff), and one page of the size real files have in two
formats."""
import numpy as np
import pytest
import torch

import tiff_write_checks as K
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
    assert K.geometry(target) == 2 * 5 + 5 + 7 * 4


def test_formats(target):
    assert K.formats(target) == 44 + 7 + 5


def test_dense_and_assemble(target):
    assert K.dense_and_assemble(target) == 2 * 4


def test_pieces(target):
    assert K.pieces(target) == 4 * 6


def test_launch_groups(target):
    """30 MiB in six strips of five 1 MiB pieces under the smallest scratch limit, 64 MiB: a piece takes its slot, 4 MiB of match scratch
    and a sixteenth of that, so the 30 pieces need at least three groups (asserted from the group size the limit gives) and strips lie
    across their borders.  Level 1 keeps it in seconds; the bytes must be those of the one group the default limit gives"""
    c = K.Case(4096, 7680, 1, 8, pred=2, rps=1280, big=True, seed=14)
    assert c.n_segs == 6 and len(c.segs[0]) == 5 << 20
    assert K.launch_group(target, 8 << 30, c, 1 << 20) >= 30                  # the default limit: one group

    def group_of(on):
        assert target.L.zmi_ctx_set_scratch_limit(target.ctx, (64 << 20) if on else (8 << 30)) == 0

    assert K.across_groups(target, c, 1 << 20, 1, K.launch_group(target, 64 << 20, c, 1 << 20), group_of, exact=False) == 1


def test_determinism(target, inf_selection):
    assert K.determinism(target, levels=(6, 1)) == 8


def test_align(target):
    assert K.aligns(target) == 8


def test_inline_arrays(target):
    assert K.inline_arrays(target) == 4


def test_arguments(target):
    assert K.arguments(target) == 30 + 8


def test_capacity(target):
    assert K.capacity(target) == 8


# ---- the Engine layer ---------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _tensor(e, c, dtype):
    return torch.from_numpy(np.frombuffer(c.image, dtype=np.uint8).copy()).to(e.device).view(dtype).view(c.height, c.width, c.samples)


@pytest.mark.parametrize("kind", ["uint8 RGB tiles", "int16 two samples strips", "float32 tiles"])
def test_engine_write_and_read_back(target, kind):
    e = target.e
    if kind.startswith("uint8"):
        c, dtype, kw = K.Case(50, 40, 3, 8, 1, 2, tile=(16, 16), seed=1), torch.uint8, dict(tile=16)
    elif kind.startswith("int16"):
        c, dtype, kw = K.Case(33, 20, 2, 16, 2, 2, rps=3, extra=1, photometric=1, seed=2), torch.int16, dict(rows_per_strip=3, extra_samples=1, align=1)
    else:
        c, dtype, kw = K.Case(37, 21, 1, 32, 3, 3, tile=(16, 32), big=True, seed=3), torch.float32, dict(tile=(16, 32), bigtiff=True)
    img = _tensor(e, c, dtype)
    if c.samples == 1:
        img = img[:, :, 0]
    out, file_len, seg_len, status = e.tiff_write(img, **kw)                 # predictor "auto"
    assert status.tolist() == [0] * (c.n_segs + 1) and int(file_len) <= e.tiff_bound((c.height, c.width, c.samples), dtype, **kw)
    f = _host(out[:int(file_len)])
    tags, segs = K.parse(f)
    K.check_tags(tags, c, kw.get("align", 16))
    assert tags[317][1] == [3 if dtype == torch.float32 else 2] and segs == c.segs_zero
    assert seg_len.tolist() == tags[325 if c.tile else 279][1]
    assert f == e.save_tiff(img, **kw)
    tf = e.tiff_directory(f)
    assert _host(tf.pages[0]) == _host(e.last_tiff_written) and tf.dtype(0) == dtype and tf.shape(0) == (c.height, c.width, c.samples)
    back, st = e.tiff_read(None, tf)
    assert st.tolist() == [0] * c.n_segs and _host(back) == c.image
    if K.HAVE_PIL and K.pil_reads(c):
        assert K.pil_pixels(f) == c.image
    # the dense form: what tiff_read(assemble=False) returns is written again, padding and all
    dense, off, ln, st = e.tiff_read(None, tf, assemble=False)
    kw2 = dict(kw, predictor=1, level=1)
    out2, len2, _, st2 = e.tiff_write((dense, off, (c.height, c.width, c.samples), dtype), **kw2)
    assert st2.tolist() == [0] * (c.n_segs + 1)
    tags2, segs2 = K.parse(_host(out2[:int(len2)]))
    assert tags2[317][1] == [1] and segs2 == c.segs_zero
    # too small a buffer: the need is reported, save_tiff raises
    small = torch.empty(int(file_len) - 1, dtype=torch.uint8, device=e.device)
    _, need, _, st3 = e.tiff_write(img, out=small, **kw)
    assert int(need) == int(file_len) and st3.tolist()[-1] == K.Z_BUF_ERROR
    with pytest.raises(RuntimeError, match="status -5"):
        e.save_tiff(img, out=small, **kw)
    with pytest.raises(ValueError):
        e.tiff_write(img, tile=24)


@pytest.mark.parametrize("kind", ["rgb8 predictor 2, tiles of 256 x 256", "float32 predictor 3, tiles of 512 x 512"])
def test_page_of_real_size(target, kind):
    """2048 - 37 by 2048 - 5 at level 1, assembled: edge tiles cropped on both sides"""
    if kind.startswith("rgb8"):
        c = K.Case(2048 - 37, 2048 - 5, 3, 8, 1, 2, tile=(256, 256), seed=5)
    else:
        c = K.Case(2048 - 37, 2048 - 5, 1, 32, 3, 3, tile=(512, 512), big=True, seed=6)
    K.run(target, c, assemble=True, level=1, pb=1 << 20)
