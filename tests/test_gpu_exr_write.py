"""The OpenEXR writer on the MI355X: the checks of tests/exr_write_checks.py over their whole matrices through the library's C ABI on
torch buffers, then the Engine layer (exr_bound, exr_write in its tensor and dict forms, save_exr) and frames of the sizes real files
have."""
import os

import numpy as np
import pytest
import torch

import exr_checks as X
import exr_write_checks as K
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


@pytest.mark.parametrize("layout", range(3), ids=["one HALF channel", "RGBA HALF", "G HALF + Z FLOAT + id UINT"])
def test_geometry(target, layout):
    """widths 1, 2, 3, 5, 17, 63, 64, 65 and 257 x heights 1, 15, 16, 17 and 33 x ZIPS, ZIP, NONE, three images a call"""
    assert K.geometry(target, layouts=K.LAYOUTS[layout:layout + 1]) == 3 * 9 * 5


def test_trips(target):
    assert K.trips(target) == 12 + 4


def test_tiles(target):
    assert K.tiles(target) == 8


def test_raw_rule(target):
    assert K.raw_rule(target) == 5


def test_pieces(target):
    assert K.pieces(target) == 8


def test_launch_groups(target):
    assert K.launch_groups(target, _set_group) == 3


def test_launch_groups_under_the_smallest_scratch_limit(target):
    """16 tiles of 512 x 512 RGBA HALF, 2 MiB and two pieces of 1 MiB each, under the smallest scratch limit, 64 MiB: a piece takes its
    slot, 4 MiB of match scratch and a sixteenth of that, so a group holds at most 12 pieces = 6 chunks and the 16 chunks need three
    groups.  Level 1 keeps it in seconds; the bytes must be those of the one group the default limit gives"""
    p = X.Exr(2048, 2048, K.RGBA, K.ZIP, tile=(512, 512), noise=(5,), seed=21, level=1)
    per_piece = PW_launch_group(target, 64 << 20)
    assert 2 <= per_piece < 32 and PW_launch_group(target, 8 << 30) >= 32
    ref = target.write([p], pb=1 << 20, level=1, align=16)
    stored = K.check(target, ref, [p], pb=1 << 20, level=1, align=16)
    assert stored[0] == [k == 5 for k in range(16)]
    assert target.L.zmi_ctx_set_scratch_limit(target.ctx, 64 << 20) == 0
    try:
        r = target.write([p], pb=1 << 20, level=1, align=16)
    finally:
        assert target.L.zmi_ctx_set_scratch_limit(target.ctx, 8 << 30) == 0
    assert (r.rc, r.off, r.len, r.status, r.guard_ok) == (0, ref.off, ref.len, ref.status, True) and r.out == ref.out


def PW_launch_group(t, limit):
    import png_write_checks as PW
    return PW.launch_group(t, limit, 1 << 20, 1 << 20)


def test_independence(target):
    assert K.independence(target) == 4 + 3


def test_pin(target):
    assert K.pin(target) == 1


def test_capacity(target):
    assert K.capacity(target) == 12


def test_arguments(target):
    assert K.arguments(target) == 32 + 8 + 3


# ---- the Engine layer -------------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _dev(e, plane):
    dt = {"<f2": torch.float16, "<f4": torch.float32, "<u4": torch.int32}[plane.dtype.str]
    return torch.from_numpy(plane.view(np.uint8).copy()).to(e.device).view(dt).view(plane.shape)


def test_engine_tensor_form_and_read_back(target):
    e = target.e
    files = [X.Exr(37, 21, K.RGBA, K.ZIP, xmin=-5, ymin=3, seed=k) for k in range(3)]
    t = torch.stack([torch.stack([_dev(e, pl) for pl in p.planes]) for p in files])
    kw = dict(channels=["A", "B", "G", "R"], origin=(-5, 3), level=6, piece_bytes=4096, align=16)
    out, off, ln, st = e.exr_write(t, **kw)
    assert st.tolist() == [0, 0, 0] and int(off[-1]) <= e.exr_bound((21, 37), [(n, torch.float16) for n in "RGBA"], 3, piece_bytes=4096)
    host = _host(out)
    blobs = [host[int(off[i]):int(off[i]) + int(ln[i])] for i in range(3)]
    for i, p in enumerate(files):
        assert blobs[i] == target.expected(p, 4096, 6, 0).blob
        assert blobs[i] == e.save_exr(t[i], **kw)
        assert e.last_exr_chunk_len.tolist() == [[s for s, _ in K.chunks(blobs[i], p)]]
    b = e.exr_headers(blobs)
    out2, off2, ln2, st2 = e.exr_write(t, **kw)
    written, wch = e.last_exr_written
    assert _host(b.images) == _host(written) and _host(b.chans[:, :4]) == _host(wch)
    assert b.channels(1) == [(n, torch.float16) for n in "ABGR"] and b.windows(2) == ((-5, 3, 31, 23), (0, 0, 36, 20))
    back, boff, blen, bst = e.exr_read(b)
    assert bst.tolist() == [0, 0, 0]
    for i in range(3):
        assert torch.equal(b.image(back, boff, i), t[i])
    # too small a buffer: the need is reported, the files in front are complete, save_exr raises
    small = torch.full((int(off[2]) + int(ln[2]) - 1,), 7, dtype=torch.uint8, device=e.device)
    o3, off3, ln3, st3 = e.exr_write(t, out=small, **kw)
    assert off3.tolist() == off.tolist() and st3.tolist() == [0, 0, K.Z_BUF_ERROR] and ln3.tolist() == ln.tolist()[:2] + [0]
    h3 = _host(o3)
    assert [h3[int(off[i]):int(off[i]) + int(ln[i])] for i in range(2)] == blobs[:2]          # (the gaps between the files keep the 7s)
    with pytest.raises(RuntimeError, match="status -5"):
        e.save_exr(t[0], out=torch.empty(100, dtype=torch.uint8, device=e.device), **kw)
    with pytest.raises(ValueError):
        e.exr_write(t, channels=["A", "B"])
    # planes of a multiple of 4 bytes under sorted names are written where they stand, with no copy; names out of order are sorted
    files = [X.Exr(16, 9, K.RGBA, K.ZIPS, seed=7 + k) for k in range(2)]
    t = torch.stack([torch.stack([_dev(e, pl) for pl in p.planes]) for p in files])
    for names, order in ((["A", "B", "G", "R"], [0, 1, 2, 3]), (["R", "G", "B", "A"], [3, 2, 1, 0])):
        out, off, ln, st = e.exr_write(t[:, order], channels=names, compression="zips", piece_bytes=4096, align=1)
        assert st.tolist() == [0, 0] and _host(out[:int(off[2])]) == b"".join(target.expected(p, 4096, 6, 0).blob for p in files)
    with pytest.raises(ValueError):
        e.exr_write(t.to(torch.float64), channels=["A", "B", "G", "R"])


def test_engine_dict_form_sorts_the_names(target):
    e = target.e
    p = X.Exr(40, 33, K.MIXED, K.ZIP, tile=(16, 16), seed=4)
    q = X.Exr(40, 33, K.MIXED, K.ZIP, tile=(16, 16), noise=(4,), seed=5)
    unsorted = [{"id": _dev(e, f.planes[2]), "Z": _dev(e, f.planes[1]), "G": _dev(e, f.planes[0])} for f in (p, q)]
    out, off, ln, st = e.exr_write(unsorted, tile=16, piece_bytes=512, align=1)
    assert st.tolist() == [0, 0] and int(off[1]) == int(ln[0])
    host = _host(out)
    for i, f in enumerate((p, q)):
        blob = host[int(off[i]):int(off[i]) + int(ln[i])]
        assert blob == target.expected(f, 512, 6, 0).blob
        ref = X.read_exr(blob)
        assert ref["channels"] == [("G", X.HALF), ("Z", X.FLOAT), ("id", X.UINT)] and ref["tiled"]
    assert [int(x) == len(raw) for x, raw in zip(e.last_exr_chunk_len[1].tolist(), q.raw)] == [k == 4 for k in range(9)]
    blob = e.save_exr(unsorted[0], compression="zips", level=1)
    b = e.exr_headers(blob)
    back, boff, _, bst = e.exr_read(b)
    assert bst.tolist() == [0] and b.record(0)["compression"] == 2
    for c, name in enumerate(("G", "Z", "id")):
        assert _host(b.channel(back, boff, 0, name)) == p.planes[c].tobytes()
    assert X.read_exr(e.save_exr(unsorted[0], compression="none"))["region"] == X.read_exr(blob)["region"]
    with pytest.raises(ValueError):
        e.exr_write([unsorted[0], {"G": unsorted[1]["G"]}])


@pytest.mark.parametrize("kind", ["one frame of 2048 x 1080 RGBA HALF", "1021 x 515 FLOAT in tiles of 256 x 256 at level 1"])
def test_frames_of_real_size(target, kind):
    if kind.startswith("one frame"):
        p, level = X.Exr(2048, 1080, K.RGBA, K.ZIP, noise=(9,), seed=6, level=1), 6
    else:
        p, level = X.Exr(1021, 515, (("Z", X.FLOAT),), K.ZIP, tile=(256, 256), xmin=-11, ymin=40, seed=7, level=1), 1
    r = target.write([p], pb=1 << 20, level=level, align=16)
    stored = K.check(target, r, [p], pb=1 << 20, level=level, align=16, exact=False)
    assert sum(stored[0]) == (1 if kind.startswith("one frame") else 0)
