"""The PNG reader on the MI355X: the checks of tests/png_checks.py over their whole matrices through the library's C ABI on torch
buffers, then the Engine layer (png_headers, PngBatch, png_decode) and both decode-kernel selections."""
import numpy as np
import pytest
import torch

import png_checks as K
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
    """heights 1, 63, 64, 65, 129 x widths 1, 63, 64, 65, row_bytes around the strip in pixels of 1, 3 and 4 bytes, row_bytes 1"""
    assert K.geometry(target) == 2 * 20 + 8 + 3 + 3 + 3


def test_formats(target):
    assert K.formats(target) == 30


def test_filters(target):
    assert K.filters(target) == 10 + 25 + 6 + 3 + 5


def test_idat_layout(target):
    assert K.idat_layout(target) == 14


@pytest.mark.parametrize("count", [1, 3, 64, 65, 300])
def test_batches(target, count):
    """every count at the input alignments 0, 1, 3, 15 with the output alignments 1, 16, 4096 in turn"""
    assert K.batches(target, counts=[count]) == 4


def test_selection_and_room(target):
    assert K.selection(target) == 14


@pytest.mark.parametrize("flags", [K.NATIVE16, 0])
def test_statuses(target, flags):
    assert K.statuses(target, flags=flags) == 38


def test_no_crc(target):
    assert K.no_crc(target) == 38


def test_scratch_limit_status(target):
    assert K.scratch(target) == 3


def test_forged_record(target):
    assert K.forged_record(target) == 3


def test_determinism(target):
    assert K.determinism(target) == 9


def test_arguments(target):
    assert K.arguments(target) == 10


def test_tall_image_spreads_over_chains(target):
    """1000 rows of adaptive filters (16 bands, a chain start in most of them) and 1000 rows of Paeth (one chain through 16 bands)"""
    pngs = [K.Png(37, 1000, 2, 8, K.adaptive(1000, 1), seed=1), K.Png(37, 1000, 2, 8, 4, seed=2), K.Png(600, 70, 6, 16, K.adaptive(70), seed=3)]
    K.run(target, pngs, align=16)


# ---- the Engine layer ---------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.cpu().numpy().tobytes()


def test_engine_batch_and_views(target):
    e = target.e
    pngs = [K.Png(13, 9, 2, 8, K.adaptive(9), seed=1), K.Png(10, 7, 0, 16, K.adaptive(7), seed=2, split=[5]),
            K.Png(11, 5, 0, 2, K.adaptive(5), seed=3), K.Png(6, 6, 3, 4, 4, seed=4, pre=K.chunk(b"tRNS", bytes([0, 128]))),
            K.Png(9, 9, 0, 8, 0, interlace=1)]
    b = e.png_headers([p.blob for p in pngs])
    assert b.n_images == 5 and b.width.tolist() == [13, 10, 11, 6, 9] and b.height.tolist() == [9, 7, 5, 6, 9]
    assert b.depth.tolist() == [8, 16, 2, 4, 8] and b.colour.tolist() == [2, 0, 0, 3, 0] and b.channels.tolist() == [3, 1, 1, 1, 1]
    assert b.status.tolist() == [0, 0, 0, 0, K.PE_INTERLACE] and b.readable.tolist() == [True] * 4 + [False]
    out, off, ln, st = e.png_decode(None, b)
    assert st.tolist() == [0, 0, 0, 0, K.Z_VERSION_ERROR] and e.last_png_detail.tolist() == [0, 0, 0, 0, K.PE_INTERLACE]
    assert ln.tolist() == [len(p.want) for p in pngs[:4]] + [0] and all(o % 16 == 0 for o in off.tolist())
    rgb = b.image(out, off, 0)
    assert rgb.shape == (9, 13, 3) and rgb.dtype == torch.uint8 and _host(rgb) == pngs[0].raw and rgb.data_ptr() == out.data_ptr() + int(off[0])
    g16 = b.image(out, off, 1)
    assert g16.shape == (7, 10, 1) and g16.dtype == torch.uint16 and g16.data_ptr() == out.data_ptr() + int(off[1])
    assert (g16.cpu().numpy().reshape(-1) == np.frombuffer(pngs[1].raw, dtype=">u2")).all()
    g2 = b.image(out, off, 2)
    assert g2.shape == (5, 3) and _host(g2) == pngs[2].raw
    want = np.unpackbits(np.frombuffer(pngs[2].raw, dtype=np.uint8).reshape(5, 3), axis=1).reshape(5, 12, 2)
    want = ((want[:, :, 0] * 2 + want[:, :, 1])[:, :11] * 85).astype(np.uint8)
    assert (b.expand(g2, 2).cpu().numpy()[:, :, 0] == want).all()
    pal = b.image(out, off, 3)
    plte, trns = b.palette(3)
    assert plte.shape == (16, 3) and trns.tolist() == [0, 128] and _host(plte) == pngs[3].blob[pngs[3].plte_pos:pngs[3].plte_pos + 48]
    rgba = b.expand(pal, 3).cpu().numpy()
    idx = np.frombuffer(pngs[3].raw, dtype=np.uint8).reshape(6, 3)
    idx = np.stack([idx >> 4, idx & 15], axis=2).reshape(6, 6)
    table = np.concatenate([plte.cpu().numpy(), np.array([[0], [128]] + [[255]] * 14, dtype=np.uint8)], axis=1)
    assert rgba.shape == (6, 6, 4) and (rgba == table[idx]).all()
    assert b.palette(0) == (None, None)
    # big-endian samples, a selection, one bytes object, a device tensor with tables
    out, off, ln, st = e.png_decode(None, b, indices=[1, 9, 1], native16=False, align=1)
    assert st.tolist() == [0, K.E_ARG, 0] and _host(out) == pngs[1].raw * 2 and off.tolist() == [0, 140, 140, 280]
    assert b.image(out, off, 2, image=1, native16=False).shape == (7, 20)
    odd = torch.empty(141, dtype=torch.uint8, device=e.device)[1:]
    if odd.data_ptr() % 2:                                                # a uint16 view of a slot at an odd address is refused, not reshaped
        e.png_decode(None, b, indices=[1], align=1, out=odd)
        with pytest.raises(ValueError, match="odd address"):
            b.image(odd, [0], 0, image=1)
    out, off, ln, st = e.png_decode(pngs[0].blob)
    assert st.tolist() == [0] and _host(out[:int(ln[0])]) == pngs[0].raw
    dev = torch.from_numpy(np.frombuffer(b"xx" + pngs[2].blob + b"yyy" + pngs[0].blob, dtype=np.uint8).copy()).to(e.device)
    b2 = e.png_headers(dev, torch.tensor([2, 5 + len(pngs[2].blob)]), torch.tensor([len(pngs[2].blob), len(pngs[0].blob)]))
    assert b2.data is dev and b2.status.tolist() == [0, 0]
    out, off, ln, st = e.png_decode(dev, b2, align=1)
    assert _host(out) == pngs[2].raw + pngs[0].raw


def test_engine_out_too_small_and_crc(target):
    e = target.e
    pngs = K.mixed(6)
    bad = K.Png(8, 8, 2, 8, 4, seed=9, bad_crc={"IDAT"})
    b = e.png_headers([p.blob for p in pngs] + [bad.blob])
    need = sum(len(p.want) for p in pngs) + len(bad.want)
    room = len(pngs[0].want) + len(pngs[1].want) + 5
    buf = torch.full((room + 64,), K.FILL, dtype=torch.uint8, device=e.device)
    out, off, ln, st = e.png_decode(None, b, out=buf[:room], align=1)
    assert out.data_ptr() == buf.data_ptr() and off.tolist()[-1] == need
    assert st.tolist() == [0, 0] + [K.Z_BUF_ERROR] * 5 and e.last_png_detail.tolist() == [0, 0] + [K.PE_OUT] * 5 and ln.tolist()[2:] == [0] * 5
    host = _host(buf)
    assert host[:room - 5] == pngs[0].bytes_out(True) + pngs[1].bytes_out(True) and host[room - 5:] == bytes([K.FILL]) * 69
    out, off, ln, st = e.png_decode(None, b, indices=[6])
    assert st.tolist() == [K.Z_DATA_ERROR] and e.last_png_detail.tolist() == [K.PE_CRC] and ln.tolist() == [0]
    out, off, ln, st = e.png_decode(None, b, indices=[6], check_crc=False)
    assert st.tolist() == [0] and _host(out[:int(ln[0])]) == bad.raw


def test_engine_both_decode_kernels(target, inf_selection):
    """300 images are one launch of up to 512 streams: the 16-wave workgroups in the product, one wave per stream under the override"""
    e = target.e
    pngs = K.mixed(300)
    out, off, ln, st = e.png_decode([p.blob for p in pngs], align=16)
    assert st.tolist() == [0] * 300 and ln.tolist() == [len(p.want) for p in pngs]
    host, off = _host(out), off.tolist()
    assert all(host[off[j]:off[j] + len(p.want)] == p.bytes_out(True) for j, p in enumerate(pngs))
