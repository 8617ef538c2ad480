"""CPU pinning of the judges of tests/tiff_checks.py: the crafter's forward predictors against the reference `unpredict` on every
format (always), and both against PIL where PIL imports with its libtiff feature -- PIL reads the crafter's files and must return
exactly their pixels, and the reference reads files PIL wrote with compression="tiff_adobe_deflate" and a predictor tag.

PIL is not a judge for, and these are left out of the PIL part only:
  * 16-bit RGB, which PIL narrows to 8 bits;
  * predictor 3 in MM files: PIL swaps the floats a second time (its result byte-swapped equals the pixels);
  * depth 64;
  * samples = 2;
  * BigTIFF in MM files: PIL tests the third header byte for the magic 43, where only II files have it."""
import io
import struct
import zlib

import numpy as np
import pytest

import tiff_checks as K


def test_crafter_against_reference():
    """every (depth, samples, predictor, byte order) of the format matrix, tiles with padding and strips with a short last one: what the
    crafter's forward predictor writes, the reference unpredict reads back (Page.stored asserts it per segment), and predictor 2 / 3
    really change the bytes"""
    n = 0
    for bits, samples, pred, be, fmt in K.format_cases():
        for kw in (dict(tile=(16, 16)), dict(rps=3)):
            p = K.Page(21, 7, samples, bits, fmt, pred, seed=bits + samples + pred, **kw)
            for k in range(p.n_segs):
                raw = zlib.decompress(p.stored(k, be))
                assert len(raw) == len(p.segs[k])
                assert K.unpredict(raw, p.rows[k], p.seg_w, samples, p.sb, pred, be) == p.segs[k]
                plain = K.predict(p.segs[k], p.rows[k], p.seg_w, samples, p.sb, 1, be)
                assert (raw == plain) == (pred == 1)
            img = np.frombuffer(p.image, dtype=np.uint8).reshape(7, 21, p.pb)
            for k in range(p.n_segs):
                r0, c0, nr, nc = p.cropped(k)
                seg = np.frombuffer(p.segs[k], dtype=np.uint8).reshape(p.rows[k], p.seg_w, p.pb)
                assert (seg[:nr, :nc] == img[r0:r0 + nr, c0:c0 + nc]).all()
            n += 1
    assert n == 2 * 88


def test_predictors_by_hand():
    """the two specifications on rows small enough to follow: predictor 2 on two RGB pixels of 16 bits in an MM file, predictor 3 on two
    float32 samples (Technical Note 3: the bytes regrouped most significant plane first, then differenced byte by byte)"""
    got = K.unpredict(struct.pack(">6H", 1, 2, 3, 0xFFFF, 10, 0x8000), 1, 2, 3, 2, 2, True)
    assert got == struct.pack("<6H", 1, 2, 3, 0, 12, 0x8003)
    a, b = struct.pack(">f", 1.5), struct.pack(">f", -2.25)                      # 3F C0 00 00, C0 10 00 00
    planes = bytes([a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3]])
    diff = bytes([planes[0]] + [(planes[i] - planes[i - 1]) & 0xFF for i in range(1, 8)])
    for be in (False, True):
        assert K.unpredict(diff, 1, 2, 1, 4, 3, be) == struct.pack("<2f", 1.5, -2.25)
        assert K.predict(struct.pack("<2f", 1.5, -2.25), 1, 2, 1, 4, 3, be) == diff


def _pil():
    try:
        from PIL import Image, features
    except ImportError:
        pytest.skip("PIL is not installed")
    if not features.check("libtiff"):
        pytest.skip("PIL was built without libtiff")
    return Image


PIL_READS = [  # (name, page arguments, file arguments, numpy dtype PIL returns)
    ("rgb predictor 2 tiles", dict(samples=3, pred=2, tile=(16, 16)), {}, "u1"),
    ("rgb predictor 2 strips", dict(samples=3, pred=2, rps=5), {}, "u1"),
    ("rgba predictor 2 tiles", dict(samples=4, pred=2, tile=(16, 32)), {}, "u1"),
    ("rgba predictor 2 strips", dict(samples=4, pred=2, rps=4), {}, "u1"),
    ("compression 32946", dict(samples=3, pred=2, rps=5, comp=32946), {}, "u1"),
    ("gray 16 MM", dict(bits=16, pred=2, rps=5), dict(be=True), "u2"),
    ("gray 16 BigTIFF", dict(bits=16, pred=2, tile=(16, 16)), dict(big=True), "u2"),
    ("gray 16 BigTIFF shuffled LONG8", dict(bits=16, pred=2, tile=(16, 16), arrays=K.LONG8), dict(big=True, shuffle=True), "u2"),
    ("rgb MM shuffled SHORT arrays", dict(samples=3, pred=2, tile=(16, 16), arrays=K.SHORT), dict(be=True, shuffle=True), "u1"),
    ("int32 predictor 2", dict(bits=32, fmt=2, pred=2, rps=5), {}, "i4"),
    ("float32 predictor 3 II", dict(bits=32, fmt=3, pred=3, tile=(16, 16)), {}, "f4"),
    ("float32 predictor 3 II strips", dict(bits=32, fmt=3, pred=3, rps=3), {}, "f4"),
    ("uncompressed", dict(samples=3, comp=1, rps=5), {}, "u1"),
    ("uncompressed MM gray 16", dict(bits=16, comp=1, rps=5), dict(be=True), "u2"),
]


@pytest.mark.parametrize("case", PIL_READS, ids=[c[0] for c in PIL_READS])
def test_pil_reads_the_crafter(case):
    Image = _pil()
    name, pkw, fkw, dt = case
    p = K.Page(37, 23, seed=7, **pkw)
    blob = K.Tiff([p], **fkw).blob
    with Image.open(io.BytesIO(blob)) as im:
        got = np.asarray(im)
    want = np.frombuffer(p.image, dtype="<" + dt).reshape(23, 37, p.samples)
    if p.samples == 1:
        want = want[:, :, 0]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.astype(want.dtype).tobytes() == want.tobytes()


def _ifd(blob):
    """the tags of the first IFD of a classic TIFF -> {tag: [values]} (SHORT, LONG and BYTE values only)"""
    e = "<" if blob[:2] == b"II" else ">"
    assert struct.unpack(e + "H", blob[2:4])[0] == 42
    at = struct.unpack(e + "I", blob[4:8])[0]
    tags = {}
    for q in range(struct.unpack(e + "H", blob[at:at + 2])[0]):
        tag, typ, cnt = struct.unpack(e + "HHI", blob[at + 2 + 12 * q:at + 10 + 12 * q])
        if typ not in K.TYPE_FMT:
            continue
        size = cnt * K.TYPE_SIZE[typ]
        pos = at + 10 + 12 * q if size <= 4 else struct.unpack(e + "I", blob[at + 10 + 12 * q:at + 14 + 12 * q])[0]
        tags[tag] = list(struct.unpack(e + "%d%s" % (cnt, K.TYPE_FMT[typ]), blob[pos:pos + size]))
    return tags, e == ">"


PIL_WRITES = [("rgb predictor 2", "u1", 3, 2), ("rgba predictor 2", "u1", 4, 2), ("gray predictor 2", "u1", 1, 2), ("gray 16 predictor 2", "u2", 1, 2),
              ("float32 predictor 3", "f4", 1, 3), ("rgb no predictor", "u1", 3, 1)]


@pytest.mark.parametrize("case", PIL_WRITES, ids=[c[0] for c in PIL_WRITES])
def test_reference_reads_pil(case):
    Image = _pil()
    name, dt, samples, pred = case
    sb = np.dtype(dt).itemsize
    px = np.frombuffer(K.samples_of(23 * 37 * samples, sb, 9), dtype="<" + dt).reshape(23, 37, samples)
    if dt == "f4":
        px = np.nan_to_num(px, nan=1.0)
    im = Image.fromarray(px[:, :, 0] if samples == 1 else px)
    f = io.BytesIO()
    im.save(f, format="TIFF", compression="tiff_adobe_deflate", tiffinfo={317: pred})
    blob = f.getvalue()
    tags, be = _ifd(blob)
    assert tags[259] == [8] and tags.get(317, [1]) == [pred] and tags[256] == [37] and tags[257] == [23] and 322 not in tags
    rps = min(tags.get(278, [23])[0], 23)
    out = b""
    for k, (off, cnt) in enumerate(zip(tags[273], tags[279])):
        rows = min(rps, 23 - k * rps)
        raw = zlib.decompress(blob[off:off + cnt])
        out += K.unpredict(raw, rows, 37, samples, sb, pred, be)
    assert out == px.astype("<" + dt).tobytes()
