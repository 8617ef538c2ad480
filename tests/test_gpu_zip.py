"""The ZIP reader on the MI355X: the checks of tests/zip_checks.py over their whole matrices through the library's C ABI on torch
buffers, then the 65 536-entry archive and the Engine layer (zip_directory, ZipDirectory, zip_read)."""
import io
import zipfile

import numpy as np
import pytest
import torch

import zip_checks as K

pytestmark = pytest.mark.gpu


class TorchMem:
    def __init__(self, device):
        self.device = device

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    class Handle:
        def __init__(self, t):
            self.t, self.ptr = t, t.data_ptr()

    def put(self, arr, shift=0):
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        buf = torch.zeros(b.size + 32, dtype=torch.uint8, device=self.device)
        at = (shift - buf.data_ptr()) % 16
        view = buf[at:at + b.size]
        if b.size:
            view.copy_(torch.from_numpy(b.copy()))
        return self.Handle(view)

    def full(self, nbytes, fill):
        return self.Handle(torch.full((nbytes,), fill, dtype=torch.uint8, device=self.device))

    def read(self, h, dtype):
        return h.t.cpu().numpy().view(dtype)


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


def test_small_shapes(target):
    assert K.small_shapes(target) == 6


@pytest.mark.parametrize("count", [3, 64, 65, 300])
def test_shapes(target, count):
    """every count at the input alignments 0, 1, 3, 15 with the output alignments 1, 16, 4096 in turn"""
    assert K.shapes(target, counts=[count]) == 4


def test_end_record(target):
    assert K.end_record(target) == 10


def test_chain_across_window_edges(target):
    """the second entry 0 .. 45 bytes in front of the window's end, and the entry of 46 + 3 x 65 535 bytes"""
    assert K.chain_edges(target) == 2 * 46
    assert K.long_entry(target) == 1


def test_chain_where_the_signature_misleads(target):
    assert K.false_guesses(target) == 9


def test_directory_sizes(target):
    assert K.directory_sizes(target) == 3


def test_zip64(target):
    assert K.zip64_extras(target) == 12


def test_local_header_differs(target):
    assert K.local_differs(target) == 4


def test_flagged_entries(target):
    assert K.flagged(target) == 13


def test_corruption(target):
    assert K.corruption(target) == 9


def test_archive_errors(target):
    assert K.archive_errors(target) == 6


def test_selection_and_room(target):
    assert K.selection(target) == 16


def test_arguments(target):
    assert K.arguments(target) == 8


def test_determinism(target):
    assert K.determinism(target) == 5


# ---- 65 536 entries: zipfile writes a ZIP64 record and a 16-bit count of 0xFFFF ----------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    b = io.BytesIO()
    datas = [b"entry %d " % i * (i % 5) for i in range(65536)]
    with zipfile.ZipFile(b, "w", zipfile.ZIP_DEFLATED) as zf:
        for i, data in enumerate(datas):
            zf.writestr("e/%05d" % i, data, zipfile.ZIP_STORED if i % 3 == 0 else zipfile.ZIP_DEFLATED)
    return b.getvalue(), datas


def test_many_entries(target, many):
    blob, datas = many
    end = len(blob) - 22
    assert blob[end:end + 4] == b"PK\x05\x06" and blob[end + 10:end + 12] == b"\xff\xff" and blob[end - 20:end - 16] == b"PK\x06\x07"
    d = target.directory(blob, cap=65536)
    assert d.rc == 0 and d.status == (0, 0) and d.canary_ok and int(d.info["n_entries"]) == 65536 == int(d.info["n_listed"])
    assert (d.listed["status"] == 0).all() and d.listed["usize"].tolist() == [len(x) for x in datas]
    r = target.inflate(d, align=16)
    assert r.rc == 0 and r.clean and r.status == [0] * 65536 and r.len == [len(x) for x in datas]
    assert all(r.slot(j) == datas[j] for j in range(65536))
    few = target.directory(blob, cap=1000)
    assert few.rc == 0 and few.status == (0, 0) and few.canary_ok and int(few.info["n_listed"]) == 1000 and int(few.info["n_entries"]) == 65536
    assert few.listed.tobytes() == d.listed[:1000].tobytes()


def test_engine_directory_grows(target, many):
    e = target.e
    blob, datas = many
    d = e.zip_directory(blob)
    assert d.n_entries == 65536 == d.info["n_entries"] and bool(d.readable.all())
    assert e.zip_directory(blob, cap=1000).n_entries == 1000
    # beyond the default cap of 65 536 the call lists again with the count it was told
    ents = [K.Ent("%x" % i, b"", method=0) for i in range(65600)]
    big = K.craft(ents, zip64=True)
    d = e.zip_directory(big)
    assert d.n_entries == 65600 and d.names()[65599] == "%x" % 65599 and d.index("10000") == 65536
    out, off, ln, st = e.zip_read(d.data, d, indices=[65599, 0])
    assert out.numel() == 0 and off.tolist() == [0, 0, 0] and st.tolist() == [0, 0]


# ---- the Engine layer ---------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.cpu().numpy().tobytes()


def test_engine_reads_npz(target):
    e = target.e
    rnd = np.random.RandomState(3)
    arrays = {"weights": rnd.randn(300, 41).astype(np.float32), "ids": np.arange(5000, dtype=np.int64) // 7, "empty": np.zeros(0, dtype=np.uint8)}
    b = io.BytesIO()
    np.savez_compressed(b, **arrays)
    blob = b.getvalue()
    out, off, ln, st = e.zip_read(blob)
    assert st.tolist() == [0, 0, 0] and e.last_zip_detail.tolist() == [0, 0, 0]
    d = e.zip_directory(blob)
    assert d.names() == [k + ".npy" for k in arrays]
    host, off, ln = _host(out), off.tolist(), ln.tolist()
    for j, (k, a) in enumerate(arrays.items()):
        npy = io.BytesIO()
        np.save(npy, a)
        assert host[off[j]:off[j] + ln[j]] == npy.getvalue(), k
        assert (np.load(io.BytesIO(host[off[j]:off[j] + ln[j]])) == a).all()


def test_engine_names_and_selection(target):
    e = target.e
    ents = [K.Ent("plain.txt", K.text(900, 1)), K.Ent("grüße/世界.txt", K.text(400, 2), flags=0x800),
            K.Ent("café.txt".encode("cp437"), K.text(100, 3), method=0), K.Ent("plain.txt", K.text(50, 4)),
            K.Ent("secret", K.text(60, 5), flags=1)]
    blob = K.craft(ents)
    assert [zi.filename for zi in zipfile.ZipFile(io.BytesIO(blob)).infolist()] == ["plain.txt", "grüße/世界.txt", "café.txt", "plain.txt", "secret"]
    dev = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(e.device)
    d = e.zip_directory(dev)
    assert d.data is dev and d.n_entries == 5 and d.info["n_entries"] == 5
    assert d.names() == ["plain.txt", "grüße/世界.txt", "café.txt", "plain.txt", "secret"]
    assert d.index("plain.txt") == 3 and d.index("café.txt") == 2
    with pytest.raises(KeyError):
        d.index("missing")
    assert d.readable.tolist() == [True, True, True, True, False] and d.status.tolist() == [0, 0, 0, 0, K.ZE_CRYPT]
    assert d.usize.tolist() == [900, 400, 100, 50, 60]
    out, off, ln, st = e.zip_read(dev, d, names=["café.txt", "grüße/世界.txt", "plain.txt"], align=16)
    assert st.tolist() == [0, 0, 0] and off.tolist() == [0, 112, 512, 576] and ln.tolist() == [100, 400, 50]
    host = _host(out)
    assert [host[o:o + l] for o, l in zip(off.tolist(), ln.tolist())] == [ents[2].data, ents[1].data, ents[3].data]
    out, off, ln, st = e.zip_read(dev, d)                                # everything: the flagged entry takes no room and raises nothing
    assert st.tolist() == [0, 0, 0, 0, K.Z_VERSION_ERROR] and e.last_zip_detail.tolist() == [0, 0, 0, 0, K.ZE_CRYPT]
    assert off.tolist() == [0, 900, 1300, 1400, 1450, 1450] and out.numel() == 1450 and _host(out) == b"".join(x.data for x in ents[:4])
    sel = torch.tensor([3, 9, 0], dtype=torch.int32, device=e.device)
    out, off, ln, st = e.zip_read(dev, d, indices=sel)
    assert st.tolist() == [0, K.E_ARG, 0] and ln.tolist() == [50, 0, 900] and _host(out) == ents[3].data + ents[0].data
    with pytest.raises(RuntimeError, match="status -3"):
        e.zip_directory(blob + b"\n")


def test_engine_out_too_small(target):
    e = target.e
    ents = K.mixed(6, big=False)
    blob = K.craft(ents)
    d = e.zip_directory(blob)
    need = sum(len(x.data) for x in ents)
    room = len(ents[0].data) + len(ents[1].data) + 5
    buf = torch.full((room + 64,), K.FILL, dtype=torch.uint8, device=e.device)
    out, off, ln, st = e.zip_read(d.data, d, out=buf[:room])
    assert out.data_ptr() == buf.data_ptr() and off.tolist()[-1] == need
    assert st.tolist() == [0, 0] + [K.Z_BUF_ERROR] * 4 and e.last_zip_detail.tolist() == [0, 0] + [K.ZE_OUT] * 4 and ln.tolist()[2:] == [0] * 4
    host = _host(buf)
    assert host[:room - 5] == ents[0].data + ents[1].data and host[room - 5:] == bytes([K.FILL]) * 69


def test_engine_both_decode_kernels(target, inf_selection):
    """300 entries are one launch of up to 512 streams: the 16-wave workgroups in the product, one wave per stream under the override"""
    e = target.e
    ents = K.mixed(300)
    blob = K.pinned(K.craft(ents), ents)
    out, off, ln, st = e.zip_read(blob, align=16)
    assert st.tolist() == [0] * 300 and ln.tolist() == [len(x.data) for x in ents]
    host, off = _host(out), off.tolist()
    assert all(host[off[j]:off[j] + len(x.data)] == x.data for j, x in enumerate(ents))
