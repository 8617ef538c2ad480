"""CPU tests of the ZIP writer (zmi_zip_bound / zmi_zip_write_dev) on the emulator build (tests/emu/, -DZMI_EMU) with the checks of
tests/zip_write_checks.py -- the ones tests/test_gpu_zip_write.py runs on the MI355X over their whole matrices.  The emulator runs a
workgroup's threads as fibers, so the matrices are thinned here to the subsets named at each test, and the archives of 65 534 and more
entries are left to the GPU.  The two judges of the checks that are code of their own -- the crafter and the file object that stands
for an archive behind a prefix -- are checked here against archives Python's zipfile wrote."""
import io
import os
import struct
import zipfile
import zlib

import numpy as np
import pytest

import zip_write_checks as K
import zmi_ctypes


class HostMem:
    """the emulator's device memory is host memory"""
    stream = None

    class Handle:
        def __init__(self, keep, view):
            self.keep, self.view, self.ptr = keep, view, view.ctypes.data

    def put(self, arr, shift=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        raw = np.zeros(b.size + 32, dtype=np.uint8)
        at = (shift - raw.ctypes.data) % 16
        view = raw[at:at + b.size]
        view[:] = b
        return self.Handle(raw, view)

    def full(self, nbytes, fill):
        return self.put(np.full(nbytes, fill, dtype=np.uint8))

    def read(self, h, dtype):
        return h.view.copy().view(dtype)


@pytest.fixture(scope="module")
def target():
    e = zmi_ctypes.Engine(zmi_ctypes.load_emu())
    yield K.Target(e.lib, e.ctx, HostMem())
    e.close()


def _setenv(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


@pytest.mark.parametrize("level,strategy", K.CONFIGS)
def test_sizes_and_pieces(target, level, strategy):
    """the seven lengths around piece_bytes 4096: level 6 as text at the four alignments and as the mix at one; every other setting
    with one kind at one alignment"""
    if (level, strategy) == (6, 0):
        assert K.shapes(target, [(6, 0)], ["text"]) == 4
        assert K.shapes(target, [(6, 0)], ["mix"], [3]) == 1
    else:
        kind = K.KINDS[K.CONFIGS.index((level, strategy)) % 4]
        assert K.shapes(target, [(level, strategy)], [kind], [15 if level else 1]) == 1


def test_small_pieces(target):
    assert K.small_pieces(target, [(0, 0), (6, 0), (6, 2)]) == 6


def test_many_pieces(target):
    assert K.many_pieces(target) == 2


def test_random_data_expands(target):
    assert K.random_expands(target) == 1


def test_names(target):
    assert K.name_shapes(target, level=0) == 3


def test_tables(target):
    assert K.tables(target, level=0) == 4


def test_grouping(target):
    assert K.grouping(target, _setenv) == 4


def test_zip64_through_base(target):
    """level 6 at the two bases around the limit, level 0 at all four"""
    assert K.zip64_base(target, levels=(6,), bases=[K.LIMIT - 100, K.LIMIT - 31]) == 2
    assert K.zip64_base(target, levels=(0,)) == 4


def test_capacity(target):
    assert K.capacity(target) == 10


def test_arguments(target):
    assert K.arguments(target) == 18 + 2 + 5 + 6 + 2


def test_determinism(target):
    assert K.determinism(target, levels=(0, 1, 6)) == 9


# ---- the judges ----------------------------------------------------------------------------------------------------------------------------
def _zipfile_archive(raws, names, method, prefix=0):
    """what zipfile writes for these entries behind `prefix` zero bytes, with the header's defaults: 1980-01-01, 0644, made on unix"""
    buf = io.BytesIO()
    buf.write(bytes(prefix))
    with zipfile.ZipFile(buf, "w") as zf:
        for raw, name in zip(raws, names):
            zi = zipfile.ZipInfo(name.decode("utf-8"), (1980, 1, 1, 0, 0, 0))
            zi.compress_type, zi.external_attr, zi.create_system = method, K.EXT0, 3
            if method == 0:
                zi.create_version = zi.extract_version = 10
            zf.writestr(zi, raw)
    return buf.getvalue()


def _deflate(raw):
    c = zlib.compressobj(-1, zlib.DEFLATED, -15)
    return c.compress(raw) + c.flush()


def test_crafter_writes_what_zipfile_writes():
    raws = K.entries_of("mix", [0, 1, 5000, 70000])
    names = [b"a", "dir/été.txt".encode("utf-8"), b"b/c/d.bin", b"same"]
    for method, pays in ((8, [_deflate(r) for r in raws]), (0, raws)):
        want = _zipfile_archive(raws, names, method)
        got = K.craft(raws, names, pays, method)
        assert got.file == want and not got.locator and not any(got.extras)
        K.check_zipfile(got.file, raws, names, method)
    # the table and info are what the positions in the file say
    cd = want.index(b"PK\x01\x02")
    assert got.info == struct.pack("<QQQQQii", 4, 4, cd, len(want) - 22 - cd, 0, 0, 0)
    at = 0
    for i, (raw, name) in enumerate(zip(raws, names)):
        row = struct.unpack_from("<QQIIIIIHHHHi", got.table, i * K.ROW)
        assert row[0] == at + 30 + len(name) and want[row[1]:row[1] + row[9]] == name and row[2:4] == (len(raw), len(raw))
        at = row[0] + len(raw)


def test_prefix_file_reads_like_the_bytes():
    raws = K.entries_of("text", [10, 3000, 0])
    names = [b"x", b"y/z", b"w"]
    whole = _zipfile_archive(raws, names, 8, prefix=1000)
    a, b = io.BytesIO(whole), K.PrefixFile(whole[1000:], 1000)
    for off, whence, n in ((0, 2, -1), (-22, 2, 22), (-30, 2, 10), (990, 0, 30), (5, 1, 4), (0, 0, 7), (2000, 0, -1), (len(whole) + 5, 0, 3)):
        assert a.seek(off, whence) == b.seek(off, whence) and a.tell() == b.tell()
        assert a.read(n) == b.read(n) and a.tell() == b.tell()
    with zipfile.ZipFile(K.PrefixFile(whole[1000:], 1000)) as zf:
        assert zf.testzip() is None and [zf.read(zi) for zi in zf.infolist()] == raws
        assert [zi.header_offset for zi in zf.infolist()][0] == 1000
    K.check_zipfile(whole[1000:], raws, names, 8, base=1000)
