"""Device-resident batch deflate / inflate on one MI355X.

torch is plumbing here: it owns the HBM buffers and the HIP stream; all compute is in the
hand-written HIP kernels of csrc/ reached through the C ABI (include/zmi355.h).

Mirrors the per-stream contract of the reference's C API
(libz-rs-sys/src/lib.rs: deflateInit2_ :2005, deflate :1281, inflateInit2_ :967, inflate :636):
every shard is compressed as deflateInit2_(level, Z_DEFLATED, wbits, 8, strategy) +
deflate(Z_FINISH) would, and the per-shard return code uses zlib's numbering.
"""
import torch

from . import _lib

WRAP_RAW, WRAP_ZLIB, WRAP_GZIP, WRAP_AUTO = 0, 1, 2, 3
GEN_SEED = 0x5A4C4942
# zmi_inflate_stream_dev detail kinds (include/zmi355.h ZMI_SI_*)
SI_CUT, SI_PIECE, SI_OUT = 3, 4, 9
BGZF_BLOCK_MAX, BGZF_HEADER, BGZF_EOF = 65280, 18, 28   # ZMI_BGZF_* (include/zmi355.h)
MM_HEADER, MM_TRUNC, MM_DATA, MM_CHECK, MM_LENGTH, MM_OUT, MM_BIG, MM_AGAIN = 1, 2, 3, 4, 5, 6, 7, 8   # ZMI_MM_* (include/zmi355.h)
# zmi_zip_directory_dev / zmi_zip_inflate_dev (include/zmi355.h ZMI_ZA_* / ZMI_ZE_*)
ZA_NOEOCD, ZA_BOUNDS, ZA_CHAIN, ZA_COUNT, ZA_ZIP64, ZA_MULTIDISK = 1, 2, 3, 4, 5, 6
ZE_LOCAL, ZE_METHOD, ZE_CRYPT, ZE_BIG, ZE_EXTRA, ZE_STORED, ZE_DATA, ZE_LENGTH, ZE_CHECK, ZE_OUT = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
ZIP_ENTRY_BYTES = 48
# zmi_png_headers_dev / zmi_png_decode_dev / zmi_png_encode_dev (include/zmi355.h ZMI_PE_* / ZMI_PNG_*)
(PE_SIGNATURE, PE_IHDR, PE_INTERLACE, PE_TRUNC, PE_CRITICAL, PE_ORDER, PE_BIG, PE_CRC, PE_DATA, PE_LENGTH, PE_FILTER, PE_OUT,
 PE_SCRATCH) = range(1, 14)
PNG_NATIVE16, PNG_NO_CRC = 1, 2
PNG_IMAGE_BYTES = 48
# zmi_tiff_directory_dev / zmi_tiff_read_dev (include/zmi355.h ZMI_TA_* / ZMI_TP_* / ZMI_TE_* / ZMI_TIFF_*)
TA_HEADER, TA_CHAIN = 1, 2
TP_TAGS, TP_FORMAT, TP_COMPRESSION, TP_PLANAR, TP_BIG, TE_OUT, TE_BOUNDS, TE_DATA, TE_LENGTH, TE_SPARSE = range(1, 11)
TIFF_ASSEMBLE = 1
TIFF_BIGTIFF = 2     # zmi_tiff_write_dev
TIFF_PAGE_BYTES, TIFF_INFO_BYTES = 72, 40
# zmi_exr_headers_dev / zmi_exr_read_dev (include/zmi355.h ZMI_XE_*)
(XE_MAGIC, XE_HEADER, XE_KIND, XE_COMPRESSION, XE_SAMPLING, XE_LEVELS, XE_CHANNELS, XE_BIG, XE_OUT, XE_SCRATCH, XE_CHUNK, XE_MISSING,
 XE_DATA, XE_LENGTH) = range(1, 15)
EXR_IMAGE_BYTES, EXR_CHANNEL_BYTES = 88, 24


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class StreamIndex:
    """Access points into ONE deflate stream (zmi_inflate_stream_index_dev, include/zmi355.h): bit int64 [n] (bit positions in the
    stream), out int64 [n + 1] (output offsets, then the total), win uint8 [n, 32768] (the output in front of every point,
    right-aligned; None: the points forget history) -- device tensors -- and max_gap, the greatest distance between two entries of
    `out`."""
    WIN = 32768

    def __init__(self, bit, out, win, max_gap):
        self.bit, self.out, self.win, self.max_gap = bit, out, win, int(max_gap)

    @property
    def n_points(self):
        return int(self.bit.numel())

    def save(self, path):
        """one .npz: bit, out, max_gap and, where there are windows, win"""
        import numpy as np
        arrays = {"bit": self.bit.cpu().numpy(), "out": self.out.cpu().numpy(), "max_gap": np.array([self.max_gap], dtype=np.int64)}
        if self.win is not None:
            arrays["win"] = self.win.cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device):
        import numpy as np
        with np.load(path) as z:
            bit, out, gap = z["bit"], z["out"], int(z["max_gap"][0])
            win = z["win"] if "win" in z.files else None
        dev = torch.device(device)
        return cls(torch.from_numpy(bit).to(dev), torch.from_numpy(out).to(dev), torch.from_numpy(win).to(dev) if win is not None else None, gap)

    @classmethod
    def from_pieces(cls, piece_off, piece_bytes, n):
        """The history-free index of deflate_stream(independent=True, index=True): piece_off is that call's index (the byte offset
        of every piece's first deflate byte, then the end of the deflate data), piece_bytes its piece size, n the length of the
        data.  Every piece starts on a byte boundary and refers to nothing in front of it, so there are no windows."""
        pieces = int(piece_off.numel()) - 1
        bit = piece_off[:pieces].to(torch.int64) * 8
        out = torch.arange(pieces + 1, dtype=torch.int64, device=piece_off.device) * int(piece_bytes)
        out[pieces] = int(n)
        return cls(bit, out, None, min(int(piece_bytes), int(n)))


class BgzfIndex:
    """The block index of a BGZF file written by Engine.bgzf_compress: block_off int64 [n_blocks + 1] (device tensor: the file offset
    of every block, then that of the end-of-file block), block_bytes (raw bytes per block, the last one may be shorter) and n, the
    length of the raw data."""

    def __init__(self, block_off, block_bytes, n):
        self.block_off, self.block_bytes, self.n = block_off, int(block_bytes), int(n)
        self._host = None

    @property
    def n_blocks(self):
        return int(self.block_off.numel()) - 1

    def _offsets(self):
        if self._host is None:
            self._host = self.block_off.tolist()
        return self._host

    def stream_index(self):
        """the window-less StreamIndex of the file: a point at the first deflate byte of every block (18 bytes behind its start)"""
        nb = self.n_blocks
        bit = (self.block_off[:nb].to(torch.int64) + BGZF_HEADER) * 8
        out = torch.arange(nb + 1, dtype=torch.int64, device=self.block_off.device) * self.block_bytes
        out[nb] = self.n
        return StreamIndex(bit, out, None, min(self.block_bytes, self.n))

    def virtual_offset(self, u):
        """htslib's virtual file offset of raw byte u: the block's file offset << 16 | the offset inside the block"""
        return self._offsets()[int(u) // self.block_bytes] << 16 | int(u) % self.block_bytes

    def save_gzi(self, path):
        """htslib's .gzi: a little-endian u64 count, then (compressed offset, uncompressed offset) u64 pairs of blocks 1 .. n_blocks - 1"""
        import struct
        off = self._offsets()
        pairs = [(off[i], i * self.block_bytes) for i in range(1, self.n_blocks)]
        with open(path, "wb") as f:
            f.write(struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs))

    @classmethod
    def load_gzi(cls, path, file_bytes, device, block_bytes=None):
        """file_bytes: the BGZF file the table belongs to (bytes or a uint8 tensor): its length gives the end-of-file block's offset,
        the ISIZE word in front of that block the length of the last block.  block_bytes is read from the first pair; a file of 0 or
        1 blocks has none, there the caller passes it."""
        import struct
        with open(path, "rb") as f:
            raw = f.read()
        count = struct.unpack_from("<Q", raw, 0)[0]
        if len(raw) != 8 + 16 * count:
            raise ValueError("%s: not a .gzi table (%d bytes for %d entries)" % (path, len(raw), count))
        words = struct.unpack_from("<%dQ" % (2 * count), raw, 8)
        size = int(file_bytes.numel()) if torch.is_tensor(file_bytes) else len(file_bytes)
        if size < BGZF_EOF:
            raise ValueError("a BGZF file is at least its %d-byte end-of-file block" % BGZF_EOF)
        if count:
            block_bytes = words[1]
        elif block_bytes is None:
            raise ValueError("a table without entries does not tell block_bytes: pass it")
        off = [0] + list(words[0::2]) + [size - BGZF_EOF]
        n = 0
        if size > BGZF_EOF:
            tail = file_bytes[size - BGZF_EOF - 4:size - BGZF_EOF]
            isize = struct.unpack("<I", bytes(tail.tolist()) if torch.is_tensor(tail) else bytes(tail))[0]
            n = count * int(block_bytes) + isize
        else:
            off = [0]
        return cls(torch.tensor(off, dtype=torch.int64, device=torch.device(device)), block_bytes, n)


class PngBatch:
    """A batch of PNG files as zmi_png_headers_dev lists them (include/zmi355.h).  data: the files on the device; offsets int64 [n] /
    lengths int32 [n]: file i is data[offsets[i] : + lengths[i]]; images: uint8 [n, 48], the device table of zmi_png_image records.
    width / height / status are int32 views of the table, depth / colour / channels int32 copies of its byte fields."""

    def __init__(self, data, offsets, lengths, images):
        self.data, self.offsets, self.lengths, self.images = data, offsets, lengths, images
        self._host = None

    @property
    def n_images(self):
        return int(self.images.shape[0])

    def _word(self, k):
        return self.images.view(torch.int32)[:, k]

    @property
    def width(self):
        return self._word(0)

    @property
    def height(self):
        return self._word(1)

    @property
    def depth(self):
        return self.images[:, 8].to(torch.int32)

    @property
    def colour(self):
        return self.images[:, 9].to(torch.int32)

    @property
    def channels(self):
        return self.images[:, 10].to(torch.int32)

    @property
    def row_bytes(self):
        return self._word(3)

    @property
    def status(self):
        """int32 [n]: 0 = readable, else the PE_* reason the headers call gives"""
        return self._word(11)

    @property
    def readable(self):
        return self.status == 0

    def record(self, j):
        """the host copy of record j as a dict (the table is copied to the host once)"""
        if self._host is None:
            self._host = self.images.cpu().numpy()
        r = self._host[j]
        w = r.view("<u4")
        return {"width": int(w[0]), "height": int(w[1]), "depth": int(r[8]), "colour": int(r[9]), "channels": int(r[10]), "bpp": int(r[11]),
                "row_bytes": int(w[3]), "idat_pos": int(w[4]), "n_idat": int(w[5]), "idat_bytes": int(w[6]), "plte_pos": int(w[7]),
                "plte_len": int(w[8]), "trns_pos": int(w[9]), "trns_len": int(w[10]), "status": int(r.view("<i4")[11])}

    def image(self, out, out_off, j, image=None, native16=True):
        """Slot j of a png_decode result as a zero-copy view of `out`: [H, W, C] uint8 for depth 8, [H, W, C] uint16 for depth 16 decoded
        with native16, [H, row_bytes] uint8 for packed depths and for big-endian 16-bit samples.  A uint16 view needs the slot at an
        even address: decoded with align=1 it may stand at an odd one, which raises ValueError (decode with align >= 2, the default
        is 16).  image: the index of the image the slot decoded (default: j, the whole batch in order)."""
        r = self.record(j if image is None else image)
        at = int(out_off[j])
        flat = out[at:at + r["height"] * r["row_bytes"]]
        if r["depth"] == 8:
            return flat.view(r["height"], r["width"], r["channels"])
        if r["depth"] == 16 and native16:
            if (out.data_ptr() + at) % 2:
                raise ValueError("image: slot %d stands at an odd address, a uint16 view needs align >= 2" % j)
            return flat.view(torch.uint16).view(r["height"], r["width"], r["channels"])
        return flat.view(r["height"], r["row_bytes"])

    def palette(self, j):
        """(PLTE as uint8 [n, 3], tRNS as uint8 [m] or None) of image j: views of the file on the device; (None, None) without PLTE"""
        r = self.record(j)
        base = int(self.offsets[j])
        if r["plte_pos"] == 0:
            return None, None
        plte = self.data[base + r["plte_pos"]:base + r["plte_pos"] + r["plte_len"]].view(-1, 3)
        trns = self.data[base + r["trns_pos"]:base + r["trns_pos"] + r["trns_len"]] if r["trns_pos"] else None
        return plte, trns

    def expand(self, img, j):
        """Plain torch indexing, no kernel: the view image() gave for image j -> [H, W, C] uint8.  Packed gray samples are unpacked and
        scaled by 255 // (2^depth - 1), as PIL scales them; palette indices of any depth become RGB, or RGBA where the file has a tRNS
        (entries beyond it are opaque); depth-8 images come back as they are; 16-bit images are not touched."""
        r = self.record(j)
        depth, colour, W = r["depth"], r["colour"], r["width"]
        if depth < 8:
            per = 8 // depth
            shifts = torch.arange(per - 1, -1, -1, device=img.device, dtype=torch.int32) * depth
            idx = ((img.to(torch.int32).unsqueeze(-1) >> shifts) & ((1 << depth) - 1)).reshape(r["height"], -1)[:, :W]
        elif depth == 8 and colour == 3:
            idx = img.reshape(r["height"], W).to(torch.int32)
        else:
            return img
        if colour == 0:
            return (idx * (255 // ((1 << depth) - 1))).to(torch.uint8).unsqueeze(-1)
        plte, trns = self.palette(j)
        table = plte
        if trns is not None:
            alpha = torch.full((plte.shape[0], 1), 255, dtype=torch.uint8, device=plte.device)
            alpha[:trns.numel(), 0] = trns[:plte.shape[0]]
            table = torch.cat([plte, alpha], dim=1)
        return table[idx.to(torch.int64).clamp(0, table.shape[0] - 1)]


class ExrBatch:
    """A batch of OpenEXR files as zmi_exr_headers_dev lists them (include/zmi355.h).  data: the files on the device; offsets int64 [n] /
    lengths int32 [n]: file i is data[offsets[i] : + lengths[i]]; images: uint8 [n, 88], the device table of zmi_exr_image records;
    chans: uint8 [n, chan_cap, 24], the zmi_exr_channel records.  Everything below reads ONE host copy of both tables, made at the
    first use (one synchronisation)."""
    _DTYPES = {0: torch.int32, 1: torch.float16, 2: torch.float32}       # UINT leaves as int32 bits

    def __init__(self, data, offsets, lengths, images, chans, chan_cap, host_data=None):
        self.data, self.offsets, self.lengths, self.images, self.chans, self.chan_cap = data, offsets, lengths, images, chans, chan_cap
        self._host_data, self._host = host_data, None

    def _tables(self):
        if self._host is None:
            import numpy as np
            img = np.dtype([("version", "<u4"), ("compression", "u1"), ("line_order", "u1"), ("tile_mode", "u1"), ("tiled", "u1"),
                            ("data_window", "<i4", 4), ("display_window", "<i4", 4), ("width", "<u4"), ("height", "<u4"),
                            ("lines_per_chunk", "<u4"), ("tile_w", "<u4"), ("tile_h", "<u4"), ("n_channels", "<u4"), ("n_chunks", "<u4"),
                            ("row_bytes", "<u4"), ("region_bytes", "<u4"), ("status", "<i4"), ("table_pos", "<u8")])
            ch = np.dtype([("name_pos", "<u4"), ("name_len", "<u4"), ("pixel_type", "<i4"), ("x_sampling", "<i4"), ("y_sampling", "<i4"),
                           ("plane_off", "<u4")])
            both = torch.cat([self.images.reshape(-1), self.chans.reshape(-1)]).cpu().numpy()
            n = self.n
            self._host = (both[:n * EXR_IMAGE_BYTES].view(img), both[n * EXR_IMAGE_BYTES:].view(ch).reshape(n, self.chan_cap),
                          self.offsets.cpu().tolist() if n else [])
        return self._host

    @property
    def n(self):
        return int(self.images.shape[0])

    def record(self, i):
        """record i as a dict of Python values"""
        r = self._tables()[0][i]
        return {k: (tuple(int(x) for x in r[k]) if r[k].ndim else int(r[k])) for k in r.dtype.names}

    def status(self, i):
        """0 = readable, else the XE_* reason the headers call gives"""
        return int(self._tables()[0][i]["status"])

    @property
    def readable(self):
        return [int(s) == 0 for s in self._tables()[0]["status"]]

    def _listed(self, i):
        return min(int(self._tables()[0][i]["n_channels"]), self.chan_cap)

    def channels(self, i):
        """[(name, dtype)] in storage order (the first chan_cap of them)"""
        rec, ch, offs = self._tables()
        out = []
        for c in range(self._listed(i)):
            at, ln = offs[i] + int(ch[i][c]["name_pos"]), int(ch[i][c]["name_len"])
            raw = bytes(self._host_data[at:at + ln]) if self._host_data is not None else bytes(self.data[at:at + ln].cpu().numpy().tobytes())
            out.append((raw.decode("latin-1"), self._DTYPES[int(ch[i][c]["pixel_type"])]))
        return out

    def shape(self, i):
        """(C, H, W)"""
        r = self._tables()[0][i]
        return int(r["n_channels"]), int(r["height"]), int(r["width"])

    def windows(self, i):
        """(dataWindow, displayWindow), each (xMin, yMin, xMax, yMax)"""
        r = self._tables()[0][i]
        return tuple(int(x) for x in r["data_window"]), tuple(int(x) for x in r["display_window"])

    def tiled(self, i):
        """(xSize, ySize) of a tiled file, None for scanlines"""
        r = self._tables()[0][i]
        return (int(r["tile_w"]), int(r["tile_h"])) if int(r["tiled"]) else None

    def image(self, out, out_off, j, file=None):
        """Slot j of an exr_read result as a zero-copy [C, H, W] view of `out` in the channels' common dtype; raises ValueError where
        the types differ.  The planes stand at multiples of 4 bytes, so with several HALF channels of an odd W * H one unwritten
        pixel lies between two planes: the view is then strided (plane stride W * H + 1), dense in every other case.  file: the index
        of the file the slot read (default: j, the whole batch in order)."""
        i = j if file is None else file
        chans = self.channels(i)
        if len({d for _, d in chans}) != 1:
            raise ValueError("image: the channels of file %d differ in type, use channel()" % i)
        c, h, w = self.shape(i)
        at = int(out_off[j])
        dt = chans[0][1]
        size = 2 if dt == torch.float16 else 4
        pitch = -(-h * w * size // 4) * 4 // size                        # a plane's pixels and its padding, as plane_off places them
        flat = out[at:at + int(self._tables()[0][i]["region_bytes"])].view(dt)
        return torch.as_strided(flat, (c, h, w), (pitch, w, 1))

    def channel(self, out, out_off, j, name, file=None):
        """channel `name` of slot j as a zero-copy [H, W] view of `out` in the channel's dtype (float16, float32, int32 bits for UINT)"""
        i = j if file is None else file
        _, h, w = self.shape(i)
        for c, (nm, dt) in enumerate(self.channels(i)):
            if nm == name:
                at = int(out_off[j]) + int(self._tables()[1][i][c]["plane_off"])
                return out[at:at + h * w * (2 if dt == torch.float16 else 4)].view(dt).view(h, w)
        raise KeyError(name)


class ZipDirectory:
    """The central directory of a ZIP archive as zmi_zip_directory_dev lists it (include/zmi355.h).  entries: uint8 [n_listed, 48], the
    device table of zmi_zip_entry records; info: the host copy of zmi_zip_info as a dict; data: the archive on the device.  The int32
    views below are slices of the table: usize / csize / crc32 are uint32 words and read negative from 2 GiB on."""

    def __init__(self, data, entries, info):
        self.data, self.entries, self.info = data, entries, info
        self._names = None

    @property
    def n_entries(self):
        return int(self.entries.shape[0])

    def _word(self, k):
        return self.entries.view(torch.int32)[:, k]

    @property
    def csize(self):
        return self._word(4)

    @property
    def usize(self):
        return self._word(5)

    @property
    def crc32(self):
        return self._word(6)

    @property
    def status(self):
        """int32 [n]: 0 = readable, else the ZE_* reason the directory gives"""
        return self._word(11)

    @property
    def readable(self):
        return self.status == 0

    def names(self):
        """The names, decoded as UTF-8 where general-purpose bit 11 is set and as cp437 elsewhere: one device-to-host copy of the
        directory's bytes and one of the table."""
        if self._names is None:
            n = self.n_entries
            if n == 0:
                self._names = []
                return self._names
            lo = int(self.info["base"] + self.info["cd_off"])
            cd = self.data[lo:lo + int(self.info["cd_size"])].cpu().numpy().tobytes()
            host = self.entries.cpu().numpy()
            name_off = host[:, 8:16].copy().view("<u8")[:, 0]
            flags = host[:, 38:40].copy().view("<u2")[:, 0]
            name_len = host[:, 40:42].copy().view("<u2")[:, 0]
            self._names = [cd[int(o) - lo:int(o) - lo + int(l)].decode("utf-8" if f & 0x800 else "cp437")
                           for o, l, f in zip(name_off, name_len, flags)]
        return self._names

    def index(self, name):
        """the index of the LAST entry of that name (the one zipfile's getinfo returns); KeyError if there is none"""
        names = self.names()
        for k in range(len(names) - 1, -1, -1):
            if names[k] == name:
                return k
        raise KeyError(name)


class TiffFile:
    """A TIFF file as zmi_tiff_directory_dev lists it (include/zmi355.h).  data: the file on the device; pages: uint8 [n, 72], the
    device table of zmi_tiff_page records; info: the host copy of zmi_tiff_info as a dict.  The table is copied to the host once, when
    the first geometry is asked for."""
    _FIELDS = [("offsets_pos", "<u8"), ("counts_pos", "<u8"), ("width", "<u4"), ("height", "<u4"), ("seg_w", "<u4"), ("seg_h", "<u4"),
               ("segs_across", "<u4"), ("segs_down", "<u4"), ("n_segs", "<u4"), ("seg_bytes", "<u4"), ("bits", "<u2"), ("samples", "<u2"),
               ("sample_format", "<u2"), ("predictor", "<u2"), ("compression", "<u2"), ("photometric", "<u2"), ("extra_samples", "<u2"),
               ("sample_bytes", "u1"), ("big_endian", "u1"), ("bigtiff", "u1"), ("tiled", "u1"), ("offsets_type", "u1"),
               ("counts_type", "u1"), ("status", "<i4")]

    def __init__(self, data, pages, info):
        self.data, self.pages, self.info = data, pages, info
        self._host = None

    @property
    def n_pages(self):
        """the pages listed (info["n_pages"]: the pages the file has)"""
        return int(self.pages.shape[0])

    @property
    def status(self):
        """int32 [n]: 0 = readable, else the TP_* reason"""
        return self.pages.view(torch.int32)[:, 17]

    @property
    def readable(self):
        return self.status == 0

    def record(self, p):
        """the host copy of record p as a dict"""
        if self._host is None:
            import numpy as np
            self._host = self.pages.cpu().numpy().view(np.dtype(self._FIELDS)).reshape(-1)
        r = self._host[p]
        return {name: int(r[name]) for name, _ in self._FIELDS}

    def shape(self, p):
        r = self.record(p)
        return (r["height"], r["width"], r["samples"])

    def tile_shape(self, p):
        """[rows, columns, samples] of a full segment: a tile, or a strip of seg_h rows"""
        r = self.record(p)
        return (r["seg_h"], r["seg_w"], r["samples"])

    def grid(self, p):
        """(segments down, segments across); segment k stands at divmod(k, across)"""
        r = self.record(p)
        return (r["segs_down"], r["segs_across"])

    def dtype(self, p):
        """the torch dtype of a sample: SampleFormat 2 signed, 3 float (16 / 32 / 64 bits), everything else unsigned"""
        r = self.record(p)
        sb = r["sample_bytes"]
        if r["sample_format"] == 3 and sb >= 2:
            return {2: torch.float16, 4: torch.float32, 8: torch.float64}[sb]
        if r["sample_format"] == 2:
            return {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}.get(sb, torch.uint8)
        return {1: torch.uint8, 2: torch.uint16, 4: torch.uint32, 8: torch.uint64}.get(sb, torch.uint8)

    def segment_bytes(self, p, k):
        """decoded bytes of segment k of page p: seg_bytes, but the rows left for the last strip; 0 for what cannot be read"""
        r = self.record(p)
        if r["status"] != 0 or not 0 <= k < r["n_segs"]:
            return 0
        rows = r["seg_h"] if r["tiled"] else min(r["seg_h"], r["height"] - (k // r["segs_across"]) * r["seg_h"])
        return rows * r["seg_w"] * r["samples"] * r["sample_bytes"]


class Engine:
    def __init__(self, device=None, scratch_bytes=None):
        if not torch.cuda.is_available():
            raise RuntimeError("zlib_rs_amd needs an MI355X (no HIP device visible); there is no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.L = _lib.lib()
        import ctypes as C
        self._ctx = C.c_void_p()
        _lib.check(self.L.zmi_ctx_create(C.byref(self._ctx), self.device.index), "zmi_ctx_create")
        self.last_png_detail = None      # png_decode: the PE_* tensor of the last call
        self.last_png_written = None     # png_encode: the table zmi_png_headers_dev would list for the files of the last call
        self.last_tiff_detail = None     # tiff_read: the TP_* / TE_* tensor of the last call
        self.last_exr_detail = None      # exr_read: the XE_* tensor of the last call (the first bad chunk above the low 8 bits)
        self.last_exr_written = None     # exr_write: (uint8 [n, 88], uint8 [n, C, 24]), the records exr_headers would list for the files
        self.last_exr_chunk_len = None   # exr_write: int32 [n, n_chunks], every chunk's dataSize
        if scratch_bytes:
            _lib.check(self.L.zmi_ctx_set_scratch_limit(self._ctx, int(scratch_bytes)), "zmi_ctx_set_scratch_limit")

    def close(self):
        if self._ctx:
            self.L.zmi_ctx_destroy(self._ctx)
            self._ctx = None

    def deflate_bound(self, n, wrap=WRAP_ZLIB, zdict=False):
        """zdict: the bound of deflate_batch(..., zdict=...), which has the DICTID in its zlib header"""
        return int((self.L.zmi_deflate_dict_bound if zdict else self.L.zmi_deflate_bound)(int(n), int(wrap)))

    # ---- synthetic benchmark shards (csrc/shardgen.h) ----
    def gen_shards(self, n_shards, shard_bytes=1 << 20, first_shard=0, seed=GEN_SEED, out=None, shard_step=1):
        """shard first_shard + i*shard_step at out[i*shard_bytes:]; shard_step = world size gives a rank its round-robin
        share of a multi-GPU job (dist.shards_of_rank)"""
        if out is None:
            out = torch.empty(n_shards * shard_bytes, dtype=torch.uint8, device=self.device)
        # the generator kernel indexes lines with 32-bit block ids: chunk very large batches
        step = 16384
        for s0 in range(0, n_shards, step):
            cnt = min(step, n_shards - s0)
            _lib.check(self.L.zmi_gen_shards_strided_dev(self._ctx, out.data_ptr() + s0 * shard_bytes, seed,
                                                         first_shard + s0 * shard_step, shard_step, cnt, shard_bytes,
                                                         _stream_ptr()), "zmi_gen_shards_strided_dev")
        return out

    # ---- the stitch: strided slots -> dense slab -> globally ordered output (csrc/pack.hip) ----
    def scan_sizes(self, lengths, out=None):
        """exclusive prefix sum of the int32 sizes -> int64 offsets, n + 1 entries (last = total)"""
        n = int(lengths.numel())
        if out is None:
            out = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        _lib.check(self.L.zmi_scan_sizes_dev(self._ctx, lengths.data_ptr(), n, out.data_ptr(), _stream_ptr()), "zmi_scan_sizes_dev")
        return out

    def pack_slab(self, slots, lengths, slab=None, offsets=None):
        """slots [n, stride] uint8 with lengths[i] valid bytes each -> (slab uint8, offsets int64[n + 1]).  Without a
        preallocated slab this synchronises once to size it."""
        n = int(lengths.numel())
        if offsets is None:
            offsets = self.scan_sizes(lengths)
        if slab is None:
            slab = torch.empty(int(offsets[n].item()) + 16, dtype=torch.uint8, device=self.device)
        self.copy_ranges(slots, None, slots.stride(0), lengths, slots.stride(0), slab, offsets)
        return slab, offsets

    def copy_ranges(self, src, src_off, src_stride, lengths, max_len, dst, dst_off):
        n = int(lengths.numel())
        _lib.check(self.L.zmi_copy_ranges_dev(self._ctx, src.data_ptr(), src_off.data_ptr() if src_off is not None else None,
                                              int(src_stride), lengths.data_ptr(), n, int(min(max_len, 0xFFFFFFFF)), dst.data_ptr(),
                                              dst_off.data_ptr(), int(dst.numel()), _stream_ptr()), "zmi_copy_ranges_dev")
        return dst

    # ---- the stitch across GPUs (csrc/exchange.hip: RCCL behind the C ABI) ----
    def comm_unique_id(self):
        """128 bytes made by one rank and carried to the others by whatever the host has (here: torch's process group)"""
        import ctypes as C
        buf = C.create_string_buffer(128)
        _lib.check(self.L.zmi_comm_unique_id(buf), "zmi_comm_unique_id")
        return buf.raw

    def comm_create(self, world, rank, uid):
        import ctypes as C
        comm = C.c_void_p()
        _lib.check(self.L.zmi_comm_create(C.byref(comm), self._ctx, int(world), int(rank), C.create_string_buffer(bytes(uid), 128)),
                   "zmi_comm_create")
        return comm

    def comm_destroy(self, comm, abort=False):
        (self.L.zmi_comm_abort if abort else self.L.zmi_comm_destroy)(comm)

    def exchange_sizes(self, comm, sizes, world):
        """all-gather of the int32 size tables -> [world, n_local] on every rank"""
        table = torch.empty((world, int(sizes.numel())), dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_exchange_sizes(comm, sizes.data_ptr(), int(sizes.numel()), table.data_ptr(), _stream_ptr()),
                   "zmi_exchange_sizes")
        return table

    def stitch_plan(self, table):
        """table [world, n_local] -> (goff [world, n_local], soff [world, n_local + 1], totals: list of world + 1 ints;
        the last one is the size of the stitched output).  Waits for the stream (the totals are host data)."""
        import ctypes as C
        world, n_local = int(table.shape[0]), int(table.shape[1])
        goff = torch.empty((world, n_local), dtype=torch.int64, device=self.device)
        soff = torch.empty((world, n_local + 1), dtype=torch.int64, device=self.device)
        d_tot = torch.empty(world + 1, dtype=torch.int64, device=self.device)
        host = (C.c_uint64 * (world + 1))()
        _lib.check(self.L.zmi_stitch_plan_dev(self._ctx, table.data_ptr(), world, n_local, goff.data_ptr(), soff.data_ptr(),
                                              d_tot.data_ptr(), host, _stream_ptr()), "zmi_stitch_plan_dev")
        return goff, soff, [int(x) for x in host]

    def exchange_round(self, comm, slab, totals, lo, chunk_bytes, stage, root=-1):
        """one bounded round of the slab exchange: stage[p] (a uint8 tensor of chunk_bytes; None for this rank, and on a rank that does
        not receive -- root >= 0 and not this rank; a receiving rank must give room for every peer: ZMI_E_ARG otherwise) receives peer p's slab bytes [lo, lo + chunk_bytes)"""
        import ctypes as C
        world = len(stage)
        tb = (C.c_uint64 * world)(*[int(t) for t in totals[:world]])
        ptrs = (C.c_void_p * world)(*[None if t is None else t.data_ptr() for t in stage])
        _lib.check(self.L.zmi_exchange_slabs_round(comm, slab.data_ptr(), tb, int(lo), int(chunk_bytes), ptrs, int(root), _stream_ptr()),
                   "zmi_exchange_slabs_round")

    # ---- deflate ----
    def deflate_batch(self, data, offsets, lengths, max_len, level=6, strategy=0, wrap=WRAP_ZLIB, out=None, out_len=None,
                      status=None, zdict=None):
        """data: uint8 device tensor; offsets (uint64 as int64) / lengths (uint32 as int32) device tensors.
        zdict: a uint8 device tensor, the one preset dictionary of every shard (deflateSetDictionary; wrap raw or zlib).
        Returns (out [n, stride] uint8, out_len [n] int32, status [n] int32)."""
        n = int(lengths.numel())
        stride = self.deflate_bound(max_len, wrap, zdict is not None)
        if out is None:
            out = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        if out_len is None:
            out_len = torch.empty(n, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        if zdict is not None:
            _check_zdict(zdict, self.device)
            _lib.check(self.L.zmi_deflate_batch_shared_dict_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                                                int(max_len), int(level), int(strategy), int(wrap),
                                                                zdict.data_ptr() if zdict.numel() else None, int(zdict.numel()),
                                                                out.data_ptr(), out.stride(0) if out.dim() == 2 else stride,
                                                                out_len.data_ptr(), status.data_ptr(), _stream_ptr()),
                       "zmi_deflate_batch_shared_dict_dev")
            return out, out_len, status
        _lib.check(self.L.zmi_deflate_batch_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                                int(max_len), int(level), int(strategy), int(wrap), out.data_ptr(),
                                                out.stride(0) if out.dim() == 2 else stride, out_len.data_ptr(),
                                                status.data_ptr(), _stream_ptr()), "zmi_deflate_batch_dev")
        return out, out_len, status

    # ---- one stream (pigz-style): the pieces of a buffer as ONE raw / zlib / gzip stream (include/zmi355.h) ----
    def stream_bound(self, n, piece_bytes=1 << 20, wrap=WRAP_GZIP):
        return int(self.L.zmi_deflate_stream_bound(int(n), int(piece_bytes), int(wrap)))

    def stream_header_bytes(self, wrap):
        return int(self.L.zmi_stream_header_bytes(int(wrap)))

    def deflate_stream(self, data, level=6, strategy=0, wrap=WRAP_GZIP, piece_bytes=1 << 20, independent=False, index=False, out=None):
        """data: uint8 device tensor -> a uint8 view of exactly the stream (and, with index=True, the int64 byte offsets in it of every
        piece's first deflate byte plus the end of the deflate data).  Carry-over pieces by default (Z_SYNC_FLUSH between them);
        independent=True: every piece forgets history (Z_FULL_FLUSH) and decodes alone.  One synchronisation, for the length."""
        n = int(data.numel())
        n_pieces = max(1, -(-n // int(piece_bytes)))
        if out is None:
            out = torch.empty(self.stream_bound(n, piece_bytes, wrap), dtype=torch.uint8, device=self.device)
        meta = torch.zeros(2, dtype=torch.int64, device=self.device)     # length | status (int32)
        idx = torch.empty(n_pieces + 1, dtype=torch.int64, device=self.device) if index else None
        _lib.check(self.L.zmi_deflate_stream_dev(self._ctx, data.data_ptr() if n else None, n, int(piece_bytes), int(level), int(strategy),
                                                 int(wrap), 1 if independent else 0, out.data_ptr(), int(out.numel()), meta.data_ptr(),
                                                 idx.data_ptr() if index else None, meta.data_ptr() + 8, _stream_ptr()),
                   "zmi_deflate_stream_dev")
        length, status = _len_status(meta)
        if status != 0:
            raise RuntimeError("zmi_deflate_stream_dev: status %d (stream of %d bytes, room for %d)" % (status, length, out.numel()))
        return (out[:length], idx) if index else out[:length]

    # ---- BGZF: blocked gzip with a block index (include/zmi355.h) ----
    def bgzf_bound(self, n, block_bytes=BGZF_BLOCK_MAX):
        return int(self.L.zmi_bgzf_bound(int(n), int(block_bytes)))

    def bgzf_compress(self, data, level=6, strategy=0, block_bytes=BGZF_BLOCK_MAX, index=False, out=None):
        """data: uint8 device tensor -> a uint8 view of exactly the BGZF file: blocks of block_bytes raw bytes, then the end-of-file
        block (and, with index=True, its BgzfIndex).  One synchronisation, for the length; a non-zero status raises."""
        n = int(data.numel())
        n_blocks = -(-n // int(block_bytes)) if 0 < int(block_bytes) <= BGZF_BLOCK_MAX else 0
        if out is None:
            out = torch.empty(self.bgzf_bound(n, block_bytes), dtype=torch.uint8, device=self.device)
        meta = torch.zeros(2, dtype=torch.int64, device=self.device)     # length | status (int32)
        idx = torch.empty(n_blocks + 1, dtype=torch.int64, device=self.device) if index else None
        _lib.check(self.L.zmi_bgzf_deflate_dev(self._ctx, data.data_ptr() if n else None, n, int(block_bytes), int(level), int(strategy),
                                               out.data_ptr() if out.numel() else None, int(out.numel()), meta.data_ptr(),
                                               idx.data_ptr() if index else None, meta.data_ptr() + 8, _stream_ptr()), "zmi_bgzf_deflate_dev")
        length, status = _len_status(meta)
        if status != 0:
            raise RuntimeError("zmi_bgzf_deflate_dev: status %d (file of %d bytes, room for %d)" % (status, length, out.numel()))
        return (out[:length], BgzfIndex(idx, block_bytes, n)) if index else out[:length]

    def bgzf_blocks(self, data, offsets, lengths, max_len, level=6, strategy=0, out=None):
        """The shards data[offsets[i] : + lengths[i]] (every length <= max_len <= 65280) as BGZF blocks, no end-of-file block: one
        rank's slab of a file.  Returns (slab: a uint8 view of exactly the blocks, block_off int64 [n + 1], block_len int32 [n]: the
        table exchange_sizes takes).  One synchronisation, for the total and the status; a non-zero status raises."""
        n = int(lengths.numel())
        if out is None:
            out = torch.empty(n * (int(max_len) + 31) + 16, dtype=torch.uint8, device=self.device)
        meta = torch.zeros(n + 2, dtype=torch.int64, device=self.device)   # block_off [n + 1] | status (int32)
        block_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_bgzf_blocks_dev(self._ctx, data.data_ptr() if data.numel() else None, offsets.data_ptr() if n else None,
                                              lengths.data_ptr() if n else None, n, int(max_len), int(level), int(strategy),
                                              out.data_ptr() if out.numel() else None, int(out.numel()), meta.data_ptr(),
                                              block_len.data_ptr() if n else None, meta.data_ptr() + 8 * (n + 1), _stream_ptr()),
                   "zmi_bgzf_blocks_dev")
        total, status = _len_status(meta[n:])
        if status != 0:
            raise RuntimeError("zmi_bgzf_blocks_dev: status %d (%d blocks, %d bytes, room for %d)" % (status, n, total, out.numel()))
        return out[:total], meta[:n + 1], block_len

    def bgzf_read_ranges(self, file, index, lo, lengths, out=None):
        """Byte ranges [lo[i], lo[i] + lengths[i]) of the raw data of the BGZF file `file` (uint8 device tensor) through its BgzfIndex
        -> (out [n, width] uint8, got int32 [n], status int32 [n]); lo and lengths are lists, numpy arrays or tensors.  A range may
        cross any number of blocks: the host splits it at the multiples of block_bytes and ONE zmi_inflate_ranges_dev call reads every
        part to its place in row i of `out` (allocated here with width = the greatest length).  A range that runs past the end of the
        data is cut there (got[i]); status[i] is 0 or the status of its first failing part."""
        import numpy as np
        to_np = lambda x: x.cpu().numpy() if torch.is_tensor(x) else np.asarray(list(x))
        lo_h = to_np(lo).astype(np.int64).reshape(-1)
        ln_h = to_np(lengths).astype(np.int64).reshape(-1)
        r = int(lo_h.size)
        bb, n = index.block_bytes, index.n
        if out is None:
            out = torch.empty((r, max(1, int(ln_h.max()) if r else 1)), dtype=torch.uint8, device=self.device)
        width = int(out.stride(0)) if out.dim() == 2 else (int(out.numel()) // r if r else 0)
        if r and int(ln_h.max()) > width:
            raise ValueError("a range of %d bytes does not fit a row of %d" % (int(ln_h.max()), width))
        got = torch.zeros(r, dtype=torch.int32, device=self.device)
        status = torch.zeros(r, dtype=torch.int32, device=self.device)
        a = np.minimum(np.maximum(lo_h, 0), n)
        b = np.minimum(a + np.maximum(ln_h, 0), n)
        first = a // bb
        cnt = np.where(b > a, (b - 1) // bb - first + 1, 0)
        parts = int(cnt.sum())
        if parts == 0:
            return out, got, status
        rid = np.repeat(np.arange(r, dtype=np.int64), cnt)
        blk = first[rid] + np.arange(parts, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        p_lo = np.maximum(a[rid], blk * bb)
        p_len = np.minimum(b[rid], (blk + 1) * bb) - p_lo
        p_off = rid * width + (p_lo - a[rid])
        dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dtype=dt, device=self.device)
        rid_d = dev(rid, torch.int64)
        _, p_got, p_st = self.read_ranges(file, index.stream_index(), dev(p_lo, torch.int64), dev(p_len, torch.int32), out=out,
                                          out_offsets=dev(p_off, torch.int64), max_len=int(p_len.max()))
        got.index_add_(0, rid_d, p_got)
        status.scatter_reduce_(0, rid_d, p_st, "amin")   # (statuses are 0 or negative)
        return out, got, status

    def find_cuts(self, data, wrap=WRAP_AUTO, min_gap=1 << 16, cap=None):
        """Proposed piece starts of a stream with flush points (the end of the header, then the byte behind every byte-aligned
        00 00 FF FF, at least min_gap bytes apart): an int64 device tensor.  One synchronisation, for the count."""
        n = int(data.numel())
        if cap is None:
            cap = max(2, n // max(1, int(min_gap)) + 2)
        cuts = torch.zeros(cap, dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_stream_find_cuts_dev(self._ctx, data.data_ptr() if n else None, n, int(wrap), int(min_gap), cuts.data_ptr(),
                                                   int(cap), cnt.data_ptr(), _stream_ptr()), "zmi_stream_find_cuts_dev")
        return cuts[:int(cnt.item())]

    def find_blocks(self, data, wrap=WRAP_AUTO, min_gap=1 << 16, cap=None):
        """Proposed piece starts of a stream WITHOUT flush points (what gzip, zlib and zlib-rs write), as BIT offsets: 8 x the end of
        the header, then the first header bit of dynamic blocks found by the block scan, at least min_gap bytes apart: an int64 device
        tensor.  One synchronisation, for the count."""
        n = int(data.numel())
        if cap is None:
            cap = max(2, n // max(1, int(min_gap)) + 2)
        cuts = torch.zeros(cap, dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_stream_find_blocks_dev(self._ctx, data.data_ptr() if n else None, n, int(wrap), int(min_gap), cuts.data_ptr(),
                                                     int(cap), cnt.data_ptr(), _stream_ptr()), "zmi_stream_find_blocks_dev")
        return cuts[:int(cnt.item())]

    def find_members(self, data, cap=None):
        """Proposed member starts of a multi-member gzip file (pack_slab's output with the gzip wrapper, BGZF, concatenated .gz files):
        0, then every offset that holds 1f 8b 08 and a FLG byte without reserved bits with at least 18 bytes behind it -- an int64
        device tensor, ascending.  Proposals may be false; inflate_members verifies them.  One synchronisation, for the count."""
        n = int(data.numel())
        grow = cap is None
        if grow:
            cap = max(1, n // 18 + 1)   # (members: an empty one is 20 bytes; proposals can be denser, see below)
        while True:
            starts = torch.zeros(cap, dtype=torch.int64, device=self.device)
            cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
            _lib.check(self.L.zmi_gzip_find_members_dev(self._ctx, data.data_ptr() if n else None, n, starts.data_ptr(), int(cap),
                                                        cnt.data_ptr(), _stream_ptr()), "zmi_gzip_find_members_dev")
            found = int(cnt.item())
            if found < cap or not grow or cap >= n // 3 + 1:
                return starts[:found]
            cap = n // 3 + 1            # a full list may be a cut one: stored 1f 8b 08 1f 8b 08 ... proposes every third byte

    def inflate_members_raw(self, data, starts, out, member_off=None):
        """One zmi_inflate_members_dev call -> (status, case, index, members, in_used, out_len), read back from the device words."""
        n = int(data.numel())
        meta = torch.zeros(4, dtype=torch.int64, device=self.device)   # out_len | in_used | members, status | detail
        mp = meta.data_ptr()
        _lib.check(self.L.zmi_inflate_members_dev(self._ctx, data.data_ptr() if n else None, n, starts.data_ptr() if starts.numel() else None,
                                                  int(starts.numel()), out.data_ptr() if out.numel() else None, int(out.numel()), mp, mp + 8,
                                                  mp + 16, member_off.data_ptr() if member_off is not None else None, mp + 20, mp + 24,
                                                  _stream_ptr()), "zmi_inflate_members_dev")
        olen, used, ms, det = meta.tolist()
        st = (ms >> 32) & 0xFFFFFFFF
        st = st - (1 << 32) if st >= 1 << 31 else st
        det &= 0xFFFFFFFF
        return st, det & 0xFF, det >> 8, ms & 0xFFFFFFFF, used, olen

    def inflate_members(self, data, starts=None, out=None, out_cap=None, index=False):
        """A multi-member gzip file -> uint8 view of the output (index=True: also the int64 output offset of every member, then the
        total).  starts: proposed member starts (find_members'; None runs it).  All members decode in one call when no two false
        proposals share a member or lie in adjacent ones; the call answers ZMI_MM_AGAIN otherwise and the loop here continues behind
        the last verified member.  Without `out` the buffer is out_cap bytes (default 4x the input + 1 MiB) and grows to the size the
        device plans when that is too small.  Any other status raises with the case and the proposal's index.  A list that ends
        early (a caller's list without the last starts, find_members with a cap) does not end the file: where the verified members
        stop on another gzip header the rest is scanned and decoded too.  self.last_members_in_used is the input offset behind the
        last member; bytes behind it (in_used < data.numel()) are not a member.  Trailing bytes that begin with 1f 8b 08 are taken
        for a member and raise if they are none, as Python's gzip does; any other trailing bytes return quietly."""
        n = int(data.numel())
        if starts is None:
            starts = self.find_members(data)
        starts = starts.to(torch.int64)
        own = out is None
        if own:
            out = torch.empty(int(out_cap) if out_cap is not None else 4 * n + (1 << 20), dtype=torch.uint8, device=self.device)
        pos = opos = 0
        offs = []
        sub = starts
        for _ in range(2 * int(starts.numel()) + 64):
            moff = torch.zeros(int(sub.numel()) + 1, dtype=torch.int64, device=self.device) if index else None
            st, kind, at, members, used, olen = self.inflate_members_raw(data[pos:], sub, out[opos:], moff)
            if kind == MM_OUT and own and opos + olen > out.numel():
                grown = torch.empty(opos + olen, dtype=torch.uint8, device=self.device)
                grown[:opos] = out[:opos]
                out = grown
                continue
            if st != 0 and kind != MM_AGAIN:
                raise RuntimeError("zmi_inflate_members_dev: status %d, case %d at proposal %d (input offset %d; %d members, %d bytes verified)"
                                   % (st, kind, at, pos + (int(sub[at]) if at < sub.numel() else 0), members, opos + olen))
            if st == 0 and pos + used + 18 <= n and members and bytes(data[pos + used:pos + used + 3].tolist()) == b"\x1f\x8b\x08":
                if index:
                    offs.append(moff[:members] + opos)
                pos += used
                opos += olen
                rest = self.find_members(data[pos:])
                starts = rest + pos
                sub = rest
                continue
            if index:
                offs.append(moff[:members] + opos)
            if st == 0:
                self.last_members_in_used = pos + used
                total = opos + olen
                if index:
                    return out[:total], torch.cat(offs + [torch.tensor([total], dtype=torch.int64, device=self.device)])
                return out[:total]
            if members == 0:
                raise RuntimeError("zmi_inflate_members_dev: ZMI_MM_AGAIN without progress at input offset %d" % pos)
            pos += used
            opos += olen
            rest = starts[starts > pos] - pos
            sub = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), rest])
        raise RuntimeError("zmi_inflate_members_dev: no result")

    def inflate_plain_stream(self, data, wrap=WRAP_AUTO, bit_index=None, min_gap=1 << 16, piece_out_max=None, out=None, out_cap=None):
        """One raw / zlib / gzip member, with or without flush points -> (uint8 view of the output, in_used).  bit_index: the piece
        starts as bit offsets (find_blocks'); None runs find_blocks(min_gap).  piece_out_max defaults to 16 x min_gap, at least
        1 MiB, at most 2^30: a piece is at least min_gap compressed bytes plus the rest of its last block, and text seldom
        shrinks below one tenth.  The loop is inflate_stream's: a cut that does not verify is dropped and the call runs again; a
        piece above piece_out_max doubles it (up to 2^30); an output above the room of `out` (default: out_cap bytes, or 4x the
        input + 1 MiB) is decoded again into a buffer of the size the device reported.  Data errors raise with the status."""
        cuts = self.find_blocks(data, wrap, min_gap) if bit_index is None else bit_index.to(torch.int64)
        if piece_out_max is None:
            piece_out_max = min(1 << 30, max(1 << 20, 16 * int(min_gap)))
        return self._inflate_stream_loop(self.L.zmi_inflate_stream_bits_dev, "zmi_inflate_stream_bits_dev", data, wrap, cuts, piece_out_max, out,
                                         out_cap)

    def inflate_stream(self, data, wrap=WRAP_AUTO, index=None, piece_out_max=1 << 20, out=None, out_cap=None):
        """One raw / zlib / gzip stream with flush points (deflate_stream's output, pigz) -> (uint8 view of the output, in_used).
        index: the piece starts (deflate_stream's index without its last entry, or find_cuts'); None runs find_cuts.  A cut that does
        not verify is dropped and the call runs again; a piece above piece_out_max doubles it; an output above the room of `out`
        (default: out_cap bytes, or 4x the input + 1 MiB) is decoded again into a buffer of the size the device reported.  Data
        errors raise with the status."""
        cuts = self.find_cuts(data, wrap) if index is None else index.to(torch.int64)
        return self._inflate_stream_loop(self.L.zmi_inflate_stream_dev, "zmi_inflate_stream_dev", data, wrap, cuts, piece_out_max, out, out_cap)

    def _inflate_stream_loop(self, fn, name, data, wrap, cuts, piece_out_max, out, out_cap):
        n = int(data.numel())
        pom = int(piece_out_max)
        if out is None:
            out = torch.empty(int(out_cap) if out_cap is not None else 4 * n + (1 << 20), dtype=torch.uint8, device=self.device)
        meta = torch.zeros(3, dtype=torch.int64, device=self.device)   # out_len | in_used | status, detail (int32)
        tries = int(cuts.numel()) + 64
        for _ in range(tries):
            meta.zero_()
            _lib.check(fn(self._ctx, data.data_ptr() if n else None, n, int(wrap), cuts.data_ptr(), int(cuts.numel()), pom, out.data_ptr(),
                          int(out.numel()), meta.data_ptr(), meta.data_ptr() + 8, meta.data_ptr() + 16, meta.data_ptr() + 20, _stream_ptr()), name)
            olen, used, sd = meta.tolist()
            st = sd & 0xFFFFFFFF
            st = st - (1 << 32) if st >= 1 << 31 else st
            det = (sd >> 32) & 0xFFFFFFFF
            kind, at = det & 0xFF, det >> 8
            if st == 0:
                self.last_piece_out_max = pom   # (what the call needed in the end: the probe tools report it)
                return out[:olen], used
            if kind == SI_CUT and 0 < at < cuts.numel():
                cuts = torch.cat([cuts[:at], cuts[at + 1:]])
            elif kind == SI_PIECE and pom < (1 << 30):
                pom = min(pom * 2, 1 << 30)
            elif kind == SI_OUT:
                out = torch.empty(olen, dtype=torch.uint8, device=self.device)
            else:
                raise RuntimeError("%s: status %d detail %d (kind %d, index %d)" % (name, st, det, kind, at))
        raise RuntimeError("%s: no result after %d attempts" % (name, tries))

    # ---- random access into one stream: index while inflating, then byte ranges (include/zmi355.h) ----
    def inflate_stream_indexed(self, data, wrap=WRAP_AUTO, bit_cuts=None, min_gap=1 << 16, span=1 << 20, piece_out_max=None, out=None,
                               out_cap=None):
        """inflate_plain_stream that also keeps a StreamIndex -> (uint8 view of the output, in_used, index): a point at the end of
        the header, then the first verified piece start at least `span` output bytes behind the point before, each with the 32 KiB
        of output in front of it.  bit_cuts: the piece starts as BIT offsets (find_blocks'; a stream with flush points passes
        8 * find_cuts(...)); None runs find_blocks(min_gap).  The loop is inflate_stream's -- a cut that does not verify is dropped, a
        piece above piece_out_max doubles it, an output above the room is decoded again into a buffer of the reported size -- with one
        synchronisation per try.  The index needs the whole output: there is no index-only build."""
        cuts = self.find_blocks(data, wrap, min_gap) if bit_cuts is None else bit_cuts.to(torch.int64)
        pom = min(1 << 30, max(1 << 20, 16 * int(min_gap))) if piece_out_max is None else int(piece_out_max)
        n = int(data.numel())
        name = "zmi_inflate_stream_index_dev"
        if out is None:
            out = torch.empty(int(out_cap) if out_cap is not None else 4 * n + (1 << 20), dtype=torch.uint8, device=self.device)
        meta = torch.zeros(5, dtype=torch.int64, device=self.device)   # out_len | in_used | status, detail (int32) | n_points (int32) | max_gap
        mp = meta.data_ptr()
        tries = int(cuts.numel()) + 64
        bufs = None
        for _ in range(tries):
            # points lie at least max(span, 1) output bytes apart
            cap = max(1, min(int(cuts.numel()), int(out.numel()) // max(int(span), 1) + 2))
            if bufs is None or bufs[0].numel() < cap:
                bufs = (torch.empty(cap, dtype=torch.int64, device=self.device), torch.empty(cap + 1, dtype=torch.int64, device=self.device),
                        torch.empty((cap, StreamIndex.WIN), dtype=torch.uint8, device=self.device))
            bit, off, win = bufs
            meta.zero_()
            _lib.check(self.L.zmi_inflate_stream_index_dev(self._ctx, data.data_ptr() if n else None, n, int(wrap), cuts.data_ptr(),
                                                           int(cuts.numel()), pom, out.data_ptr() if out.numel() else None, int(out.numel()), mp,
                                                           mp + 8, mp + 16, mp + 20, int(span), bit.data_ptr(), off.data_ptr(), win.data_ptr(),
                                                           int(bit.numel()), mp + 24, mp + 32, _stream_ptr()), name)
            olen, used, sd, pts, gap = meta.tolist()
            st = sd & 0xFFFFFFFF
            st = st - (1 << 32) if st >= 1 << 31 else st
            det = (sd >> 32) & 0xFFFFFFFF
            kind, at = det & 0xFF, det >> 8
            if st == 0:
                self.last_piece_out_max = pom
                k = pts & 0xFFFFFFFF
                return out[:olen], used, StreamIndex(bit[:k], off[:k + 1], win[:k], gap)
            if kind == SI_CUT and 0 < at < cuts.numel():
                cuts = torch.cat([cuts[:at], cuts[at + 1:]])
            elif kind == SI_PIECE and pom < (1 << 30):
                pom = min(pom * 2, 1 << 30)
            elif kind == SI_OUT:
                out = torch.empty(olen, dtype=torch.uint8, device=self.device)
            else:
                raise RuntimeError("%s: status %d detail %d (kind %d, index %d)" % (name, st, det, kind, at))
        raise RuntimeError("%s: no result after %d attempts" % (name, tries))

    def read_ranges(self, data, index, lo, lengths, out=None, out_offsets=None, max_len=None):
        """Byte ranges [lo[i], lo[i] + lengths[i]) of the OUTPUT of the stream `data`, through its StreamIndex -> (out, got int32 [n],
        status int32 [n]).  lo (int64) and lengths (int32) are device tensors or lists.  Range i lands at out_offsets[i] (int64 device
        tensor) of `out`, or in row i of the [n, max_len] buffer this call allocates; got[i] counts its bytes (less than asked where
        the stream ends), status[i] is 0, Z_DATA_ERROR, Z_BUF_ERROR or -103 (include/zmi355.h); a range with a non-zero status writes
        nothing.  No check value is verified.  max_len bounds every length (it sizes the scratch); None takes the row length of `out`,
        or reads the greatest length from the device when `out` is not given -- the only synchronisation of this call."""
        if not torch.is_tensor(lo):
            lo = torch.tensor(list(lo), dtype=torch.int64, device=self.device)
        if not torch.is_tensor(lengths):
            if max_len is None and out is None:
                max_len = max(list(lengths) + [1])
            lengths = torch.tensor(list(lengths), dtype=torch.int32, device=self.device)
        n = int(lengths.numel())
        got = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        if out is None:
            if max_len is None:
                max_len = max(1, int(lengths.max().item())) if n else 1
            out = torch.empty((n, int(max_len)), dtype=torch.uint8, device=self.device)
        stride = 0
        if out_offsets is None:
            stride = int(out.stride(0)) if out.dim() == 2 else (int(out.numel()) // n if n else 0)
        if max_len is None:
            max_len = stride if out_offsets is None else int(out.numel())
        max_len = max(1, min(int(max_len), 1 << 30))
        if n == 0:
            return out, got, status
        nd = int(data.numel())
        _lib.check(self.L.zmi_inflate_ranges_dev(self._ctx, data.data_ptr() if nd else None, nd, index.bit.data_ptr(), index.out.data_ptr(),
                                                 index.win.data_ptr() if index.win is not None and index.win.numel() else None,
                                                 index.n_points, int(index.max_gap), lo.data_ptr(), lengths.data_ptr(), n, max_len,
                                                 out.data_ptr(), out_offsets.data_ptr() if out_offsets is not None else None, stride,
                                                 got.data_ptr(), status.data_ptr(), _stream_ptr()), "zmi_inflate_ranges_dev")
        return out, got, status

    def deflate_pieces(self, data, offsets, lengths, max_len, level=6, strategy=0, wrap=WRAP_GZIP, independent=True, final=True):
        """One rank's pieces of a single stream: (slots [n, stride] uint8, sizes int32 [n], checks int32 [n], status int32 [n])."""
        n = int(lengths.numel())
        stride = int(self.L.zmi_deflate_pieces_stride(int(max_len)))
        slots = torch.empty((max(n, 1), stride), dtype=torch.uint8, device=self.device)
        sizes = torch.zeros(n, dtype=torch.int32, device=self.device)
        checks = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_deflate_pieces_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, int(max_len),
                                                 int(level), int(strategy), int(wrap), 1 if independent else 0, 1 if final else 0,
                                                 slots.data_ptr(), stride, sizes.data_ptr(), checks.data_ptr(), status.data_ptr(),
                                                 _stream_ptr()), "zmi_deflate_pieces_dev")
        return slots, sizes, checks, status

    def checksum_combine(self, checks, lengths, wrap=WRAP_GZIP, world=1):
        """(check, raw length) pairs -> (check int32 [1], total length int64 [1]) of the concatenation, on the device.  With world > 1
        the tables are rank-major ([world, n_local]: entry [r, j] is piece j * world + r), as dist's all-gathered tables are."""
        n = int(lengths.numel())
        c = torch.empty(1, dtype=torch.int32, device=self.device)
        t = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(self.L.zmi_checksum_combine_dev(self._ctx, int(wrap), checks.data_ptr() if n else None, lengths.data_ptr() if n else None,
                                                   int(world), n // int(world), c.data_ptr(), t.data_ptr(), _stream_ptr()),
                   "zmi_checksum_combine_dev")
        return c, t

    def stream_frame(self, out, payload_len, check, raw_len, wrap=WRAP_GZIP, level=6, strategy=0, out_cap=None):
        """header and trailer around the payload_len (int64 device word) bytes of deflate data at out[header:]; returns the int64
        [2] device words length | status.  out_cap: the room the stream may take (default: all of `out`; an empty view of a tensor
        has no address to pass, so a capacity of 0 is given this way)"""
        meta = torch.zeros(2, dtype=torch.int64, device=self.device)
        _lib.check(self.L.zmi_stream_frame_dev(self._ctx, int(wrap), int(level), int(strategy), payload_len.data_ptr(),
                                               check.data_ptr() if check is not None else None,
                                               raw_len.data_ptr() if raw_len is not None else None, out.data_ptr(),
                                               int(out.numel() if out_cap is None else min(out_cap, out.numel())),
                                               meta.data_ptr(), meta.data_ptr() + 8, _stream_ptr()), "zmi_stream_frame_dev")
        return meta

    # ---- inflate ----
    def inflate_batch(self, data, offsets, lengths, out, out_offsets, out_caps, wrap=WRAP_ZLIB, out_len=None, status=None, zdict=None,
                      in_used=None, detail=None):
        """zdict: a uint8 device tensor, the one preset dictionary of every stream (inflateSetDictionary; wrap raw or zlib); in_used /
        detail (int32 [n], with zdict only) receive the consumed input bytes and why a stream stopped"""
        n = int(lengths.numel())
        if out_len is None:
            out_len = torch.empty(n, dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        # inflate keeps 1 bit of scratch per byte of output capacity; the capacities are device data, `out` bounds them
        _lib.check(self.L.zmi_ctx_set_inflate_out_limit(self._ctx, int(out.numel()) + (1 << 20)), "zmi_ctx_set_inflate_out_limit")
        if zdict is not None:
            _check_zdict(zdict, self.device)
            _lib.check(self.L.zmi_inflate_batch_shared_dict_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                                                int(wrap), zdict.data_ptr() if zdict.numel() else None, int(zdict.numel()),
                                                                out.data_ptr(), out_offsets.data_ptr(), out_caps.data_ptr(),
                                                                out_len.data_ptr(), status.data_ptr(),
                                                                in_used.data_ptr() if in_used is not None else None,
                                                                detail.data_ptr() if detail is not None else None, _stream_ptr()),
                       "zmi_inflate_batch_shared_dict_dev")
            return out_len, status
        _lib.check(self.L.zmi_inflate_batch_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n,
                                                int(wrap), out.data_ptr(), out_offsets.data_ptr(), out_caps.data_ptr(),
                                                out_len.data_ptr(), status.data_ptr(), _stream_ptr()),
                   "zmi_inflate_batch_dev")
        return out_len, status

    # ---- batch inflate without an output size table ----
    def inflate_sizes(self, data, offsets, lengths, wrap=WRAP_ZLIB, hist=0, size_limit=0, in_used=None, detail=None):
        """(sizes int32 [n], status int32 [n]) of zmi_inflate_sizes_dev: what every stream would decode to, found by the decode kernel
        counting instead of storing (no output buffer, no check values).  The words are uint32: a size of 2 GiB or more reads negative
        in the int32 tensor.  hist: bytes of preset dictionary every stream may reach; size_limit 0: 2^32 - 1.  No synchronisation."""
        n = int(lengths.numel())
        sizes = torch.empty(n, dtype=torch.int32, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        _lib.check(self.L.zmi_inflate_sizes_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, int(wrap), int(hist),
                                                int(size_limit), sizes.data_ptr(), status.data_ptr(),
                                                in_used.data_ptr() if in_used is not None else None,
                                                detail.data_ptr() if detail is not None else None, _stream_ptr()),
                   "zmi_inflate_sizes_dev")
        return sizes, status

    def inflate_batch_packed(self, data, offsets, lengths, wrap=WRAP_ZLIB, zdict=None, size_limit=0, align=1, out=None, in_used=None,
                             detail=None):
        """(out, out_offsets int64 [n + 1], out_len int32 [n], status int32 [n]): the batch decoded densely into one buffer, stream i at
        out_offsets[i] (the sizes in front of it, each rounded up to `align`), out_offsets[n] = the room the whole batch needs.
        With `out` given this is zmi_inflate_batch_packed_dev as it stands: no synchronisation; where out_offsets[n] > out.numel() the
        streams that do not fit report Z_BUF_ERROR with length 0 and the caller calls again with that much room.
        With out=None the size pass and the plan run first, ONE word -- the total -- is read by the host (the one synchronisation), the
        buffer is allocated exactly, and the ordinary inflate_batch runs with the planned table: no stream is decoded for its size twice
        (in_used / detail are then filled as inflate_batch fills them: with zdict only)."""
        n = int(lengths.numel())
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        if zdict is not None:
            _check_zdict(zdict, self.device)
        out_len = torch.empty(n, dtype=torch.int32, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        if out is not None:
            out_offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            _lib.check(self.L.zmi_inflate_batch_packed_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, int(wrap),
                                                           zdict.data_ptr() if zdict is not None and zdict.numel() else None,
                                                           int(zdict.numel()) if zdict is not None else 0, int(size_limit), int(align),
                                                           out.data_ptr(), int(out.numel()), out_offsets.data_ptr(), out_len.data_ptr(),
                                                           status.data_ptr(), in_used.data_ptr() if in_used is not None else None,
                                                           detail.data_ptr() if detail is not None else None, _stream_ptr()),
                       "zmi_inflate_batch_packed_dev")
            return out, out_offsets, out_len, status
        hist = min(int(zdict.numel()), 32768) if zdict is not None else 0
        sizes, _ = self.inflate_sizes(data, offsets, lengths, wrap=wrap, hist=hist, size_limit=size_limit)
        room = ((sizes.to(torch.int64) & 0xFFFFFFFF) + (align - 1)) & ~(align - 1)
        out_offsets = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(room, 0, out=out_offsets[1:])
        total = int(out_offsets[n].item()) if n else 0
        out = torch.empty(total, dtype=torch.uint8, device=self.device)
        if n:
            self.inflate_batch(data, offsets, lengths, out, out_offsets, sizes, wrap=wrap, out_len=out_len, status=status,
                               zdict=zdict if zdict is not None and zdict.numel() else None, in_used=in_used, detail=detail)
        return out, out_offsets, out_len, status

    # ---- ZIP archives ----
    def _zip_data(self, data):
        if isinstance(data, torch.Tensor):
            if data.dtype != torch.uint8 or data.device != self.device or not data.is_contiguous():
                raise ValueError("data must be a contiguous uint8 tensor on %s" % (self.device,))
            return data
        import numpy as np
        host = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).view(np.uint8)
        return torch.from_numpy(host.reshape(-1).copy()).to(self.device)

    def zip_directory(self, data, cap=None):
        """The directory of the ZIP archive `data` (a uint8 device tensor, or bytes / numpy, which are uploaded) -> ZipDirectory.  cap:
        entries to make room for; the default, min((len - 22) // 76, 65536), holds any archive of up to 65 536 entries (an entry costs at
        least 30 + 46 bytes), and a larger archive is listed again with the count the first call reports.  One synchronisation per call:
        reading zmi_zip_info.  An archive the call refuses (ZA_*) raises; flagged entries (ZE_*) are listed and do not."""
        data = self._zip_data(data)
        n = int(data.numel())
        grow = cap is None
        if grow:
            cap = min(max(0, (n - 22) // 76), 65536)
        while True:
            entries = torch.empty((cap, ZIP_ENTRY_BYTES), dtype=torch.uint8, device=self.device)
            meta = torch.zeros(6, dtype=torch.int64, device=self.device)
            _lib.check(self.L.zmi_zip_directory_dev(self._ctx, data.data_ptr() if n else None, n, entries.data_ptr() if cap else None, int(cap),
                                                    meta.data_ptr(), _stream_ptr()), "zmi_zip_directory_dev")
            n_entries, n_listed, cd_off, cd_size, base, sd = meta.tolist()
            st = sd & 0xFFFFFFFF
            info = {"n_entries": n_entries, "n_listed": n_listed, "cd_off": cd_off, "cd_size": cd_size, "base": base,
                    "status": st - (1 << 32) if st >= 1 << 31 else st, "detail": (sd >> 32) & 0xFFFFFFFF}
            if info["status"] != 0:
                raise RuntimeError("zmi_zip_directory_dev: status %d (case %d, index %d)" % (info["status"], info["detail"] & 0xFF,
                                                                                             info["detail"] >> 8))
            if n_entries <= cap or not grow:
                return ZipDirectory(data, entries[:n_listed], info)
            cap = n_entries

    def zip_read(self, data, directory=None, names=None, indices=None, align=1, out=None):
        """Entries of a ZIP archive, inflated (or copied, where stored) densely into one buffer and checked against the directory's
        lengths and CRC-32s -> (out, out_off int64 [n_sel + 1], out_len int32 [n_sel], status int32 [n_sel]).  Slot j stands at
        out[out_off[j] : out_off[j] + out_len[j]]; out_off[-1] is the room the selection needs.  names or indices (a list or an int32
        device tensor) select; neither: every listed entry.  status 0: length and CRC-32 match; every other status (Z_DATA_ERROR,
        Z_BUF_ERROR where `out` was too small, Z_VERSION_ERROR for an entry the directory flagged) has length 0 -- nothing is raised for
        an entry.  last_zip_detail keeps the ZE_* tensor.  out=None allocates the sum of the selected usize and reads ONE word,
        out_off[-1], to check the guess (it is exact unless a selected entry is flagged)."""
        data = self._zip_data(data)
        d = directory if directory is not None else self.zip_directory(data)
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        if names is not None:
            indices = [d.index(nm) for nm in names]
        sel = None
        if indices is not None:
            sel = indices if isinstance(indices, torch.Tensor) else torch.tensor(list(indices), dtype=torch.int32, device=self.device)
            sel = sel.to(device=self.device, dtype=torch.int32).contiguous()
        n_sel = int(sel.numel()) if sel is not None else d.n_entries
        out_off = torch.zeros(n_sel + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        status = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        detail = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        self.last_zip_detail = detail

        def call(buf):
            _lib.check(self.L.zmi_zip_inflate_dev(self._ctx, data.data_ptr() if data.numel() else None, int(data.numel()),
                                                  d.entries.data_ptr() if d.n_entries else None, d.n_entries,
                                                  sel.data_ptr() if sel is not None and n_sel else None, n_sel, int(align),
                                                  buf.data_ptr() if buf.numel() else None, int(buf.numel()), out_off.data_ptr(),
                                                  out_len.data_ptr(), status.data_ptr(), detail.data_ptr(), _stream_ptr()),
                       "zmi_zip_inflate_dev")

        if out is not None:
            call(out)
            return out, out_off, out_len, status
        if n_sel == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device), out_off, out_len, status
        usize = d.usize.to(torch.int64) & 0xFFFFFFFF
        if sel is not None:
            usize = usize[sel.to(torch.int64).clamp(0, max(0, d.n_entries - 1))] if d.n_entries else usize[:0]
        guess = int((((usize + (align - 1)) // align) * align).sum().item())
        out = torch.empty(guess, dtype=torch.uint8, device=self.device)
        call(out)
        need = int(out_off[n_sel].item())
        if need > guess:      # (cannot happen: flagged entries and bad indices take no room)
            out = torch.empty(need, dtype=torch.uint8, device=self.device)
            call(out)
        return out[:need], out_off, out_len, status

    # ---- PNG images (include/zmi355.h) ----
    def png_headers(self, data, offsets=None, lengths=None):
        """The chunk chains of a batch of PNG files -> PngBatch.  data: a uint8 device tensor with offsets / lengths (int64 / int32
        tables, file i = data[offsets[i] : + lengths[i]]; neither: the tensor is ONE file), one bytes object, or a list of bytes, which
        is concatenated and uploaded.  No synchronisation; a file the call flags (PE_*) is listed and raises nothing."""
        if isinstance(data, (list, tuple)):
            import numpy as np
            offs = np.zeros(len(data), dtype=np.int64)
            if len(data) > 1:
                np.cumsum([len(b) for b in data[:-1]], out=offs[1:])
            offsets = torch.from_numpy(offs)
            lengths = torch.tensor([len(b) for b in data], dtype=torch.int32)
            data = b"".join(bytes(b) for b in data)
        data = self._zip_data(data)
        if offsets is None:
            offsets = torch.zeros(1, dtype=torch.int64)
            lengths = torch.tensor([int(data.numel())], dtype=torch.int32)
        offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
        lengths = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(lengths.numel())
        if int(offsets.numel()) < n:
            raise ValueError("png_headers: %d lengths need %d offsets" % (n, n))
        images = torch.zeros((n, PNG_IMAGE_BYTES), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.zmi_png_headers_dev(self._ctx, data.data_ptr() if data.numel() else None, offsets.data_ptr() if n else None,
                                              lengths.data_ptr() if n else None, n, images.data_ptr() if n else None, _stream_ptr()),
                   "zmi_png_headers_dev")
        return PngBatch(data, offsets, lengths, images)

    def png_decode(self, data, batch=None, indices=None, align=16, native16=True, check_crc=True, out=None):
        """Images of a batch of PNG files, inflated and unfiltered densely into one buffer -> (out, out_off int64 [n_sel + 1], out_len
        int32 [n_sel], status int32 [n_sel]).  Slot j stands at out[out_off[j] : out_off[j] + out_len[j]] as height * row_bytes bytes
        (PngBatch.image gives the view); out_off[-1] is the room the selection needs.  batch: the PngBatch of png_headers (None: made
        here from data; with a batch, data may be None); indices (a list or an int32 device tensor) select, None: every image.  status
        0: every check passed; every other status has length 0 and nothing is raised for an image.  last_png_detail keeps the PE_*
        tensor.  native16: 16-bit samples leave little-endian; check_crc=False skips the chunk CRC-32s.  out=None allocates the sum of
        the selected regions, which is ONE word read by the host."""
        b = batch if batch is not None else self.png_headers(data)
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        sel = None
        if indices is not None:
            sel = indices if isinstance(indices, torch.Tensor) else torch.tensor(list(indices), dtype=torch.int32, device=self.device)
            sel = sel.to(device=self.device, dtype=torch.int32).contiguous()
        n = b.n_images
        n_sel = int(sel.numel()) if sel is not None else n
        out_off = torch.zeros(n_sel + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        status = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        detail = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        self.last_png_detail = detail
        flags = (PNG_NATIVE16 if native16 else 0) | (0 if check_crc else PNG_NO_CRC)

        def call(buf):
            _lib.check(self.L.zmi_png_decode_dev(self._ctx, b.data.data_ptr() if n else None, b.offsets.data_ptr() if n else None,
                                                 b.lengths.data_ptr() if n else None, b.images.data_ptr() if n else None, n,
                                                 sel.data_ptr() if sel is not None and n_sel else None, n_sel, flags, int(align),
                                                 buf.data_ptr() if buf.numel() else None, int(buf.numel()), out_off.data_ptr(),
                                                 out_len.data_ptr(), status.data_ptr(), detail.data_ptr(), _stream_ptr()),
                       "zmi_png_decode_dev")

        if out is not None:
            call(out)
            return out, out_off, out_len, status
        if n_sel == 0 or n == 0:
            if n_sel:
                call(torch.empty(0, dtype=torch.uint8, device=self.device))
            return torch.empty(0, dtype=torch.uint8, device=self.device), out_off, out_len, status
        size = (b.height.to(torch.int64) & 0xFFFFFFFF) * (b.row_bytes.to(torch.int64) & 0xFFFFFFFF) * b.readable.to(torch.int64)
        if sel is not None:
            inside = (sel >= 0) & (sel < n)
            size = size[sel.to(torch.int64).clamp(0, n - 1)] * inside.to(torch.int64)
        guess = int((((size + (align - 1)) // align) * align).sum().item())
        out = torch.empty(guess, dtype=torch.uint8, device=self.device)
        call(out)
        return out, out_off, out_len, status

    # ---- TIFF files (include/zmi355.h) ----
    def tiff_directory(self, data, cap=None):
        """The IFD chain of the TIFF file `data` (a uint8 device tensor, or bytes / numpy, which are uploaded) -> TiffFile.  cap: pages
        to make room for; the default, 64, is raised to the count the first call reports where the file has more.  One
        synchronisation per call: the info is read; a file whose header or chain is broken raises."""
        data = self._zip_data(data)
        n = int(data.numel())
        grow = cap is None
        cap = 64 if cap is None else int(cap)
        while True:
            pages = torch.zeros((cap, TIFF_PAGE_BYTES), dtype=torch.uint8, device=self.device)
            meta = torch.zeros(TIFF_INFO_BYTES // 8, dtype=torch.int64, device=self.device)
            _lib.check(self.L.zmi_tiff_directory_dev(self._ctx, data.data_ptr() if n else None, n, pages.data_ptr() if cap else None, cap,
                                                     meta.data_ptr(), _stream_ptr()), "zmi_tiff_directory_dev")
            n_pages, n_listed, first, eb, sd = meta.tolist()
            st = sd & 0xFFFFFFFF
            info = {"n_pages": n_pages, "n_listed": n_listed, "first_ifd": first, "big_endian": eb & 0xFFFFFFFF, "bigtiff": (eb >> 32) & 0xFFFFFFFF,
                    "status": st - (1 << 32) if st >= 1 << 31 else st, "detail": (sd >> 32) & 0xFFFFFFFF}
            if info["status"] != 0:
                raise RuntimeError("zmi_tiff_directory_dev: status %d (case %d, IFD %d)" % (info["status"], info["detail"] & 0xFF,
                                                                                           info["detail"] >> 8))
            if n_pages <= cap or not grow:
                return TiffFile(data, pages[:n_listed], info)
            cap = n_pages

    def tiff_read(self, data, tf=None, page=0, segments=None, assemble=True, align=16, out=None):
        """Strips or tiles of one page of a TIFF file, inflated (or copied, compression 1), the predictor undone, every sample
        little-endian.  tf: the TiffFile of tiff_directory (None: made here from data; with it, data may be None); segments (a list or
        an int32 device tensor) select, None: every segment of the page.  assemble=True -> (image, status): the page as one [H, W, C]
        tensor in the page's dtype -- every selected segment at its place, cropped at the edges; what no selected segment covers is
        zero in a tensor allocated here and untouched in `out` -- and status int32 [n_sel].  assemble=False -> (out, out_off int64
        [n_sel + 1], out_len int32 [n_sel], status) as png_decode returns them: slot j is the whole segment, padding included, a
        [rows, seg_w, C] tensor at out[out_off[j] : out_off[j] + out_len[j]].  status 0: every check passed; nothing is raised for a
        segment or for a page the directory flagged (Z_DATA_ERROR / Z_VERSION_ERROR in every slot).  last_tiff_detail keeps the TP_* /
        TE_* tensor (TE_SPARSE with status 0: a segment of byte count 0, all zeros).  out: a contiguous uint8 tensor."""
        t = tf if tf is not None else self.tiff_directory(data)
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        if out is not None and (out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError("tiff_read: out must be a contiguous uint8 tensor on %s" % (self.device,))
        page = int(page)
        r = t.record(page) if 0 <= page < t.n_pages else None
        ok = r is not None and r["status"] == 0
        sel = None
        if segments is not None:
            sel = segments if isinstance(segments, torch.Tensor) else torch.tensor(list(segments), dtype=torch.int32, device=self.device)
            sel = sel.to(device=self.device, dtype=torch.int32).contiguous()
        n_sel = int(sel.numel()) if sel is not None else (r["n_segs"] if ok else 1)
        if not ok:
            decoded, sizes = 0, [0] * n_sel
        elif sel is None:
            sizes = [t.segment_bytes(page, k) for k in range(n_sel)] if not r["tiled"] else [r["seg_bytes"]] * n_sel
            decoded = sum(sizes)
        elif isinstance(segments, torch.Tensor):
            sizes, decoded = None, n_sel * r["seg_bytes"]                 # (a bound: the indices stay on the device)
        else:
            sizes = [t.segment_bytes(page, int(k)) for k in segments]
            decoded = sum(sizes)
        out_off = torch.zeros(n_sel + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        status = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        detail = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        self.last_tiff_detail = detail

        def call(buf):
            _lib.check(self.L.zmi_tiff_read_dev(self._ctx, t.data.data_ptr() if t.data.numel() else None, int(t.data.numel()),
                                                t.pages.data_ptr() if t.n_pages else None, t.n_pages, page,
                                                sel.data_ptr() if sel is not None and n_sel else None, n_sel, int(decoded),
                                                TIFF_ASSEMBLE if assemble else 0, int(align), buf.data_ptr() if buf.numel() else None,
                                                int(buf.numel()), out_off.data_ptr(), out_len.data_ptr(), status.data_ptr(), detail.data_ptr(),
                                                _stream_ptr()), "zmi_tiff_read_dev")

        if assemble:
            size = r["height"] * r["width"] * r["samples"] * r["sample_bytes"] if ok else 0
            if out is None:
                out = (torch.zeros if sel is not None else torch.empty)(size, dtype=torch.uint8, device=self.device)
            call(out)
            if not ok or int(out.numel()) < size:
                return out[:0], status
            return out[:size].view(t.dtype(page)).view(t.shape(page)), status
        if out is None:
            guess = n_sel * (-(-r["seg_bytes"] // align) * align) if sizes is None else sum(-(-s // align) * align for s in sizes)
            out = torch.empty(guess if ok else 0, dtype=torch.uint8, device=self.device)
        call(out)
        return out, out_off, out_len, status

    # ---- OpenEXR images (include/zmi355.h) ----
    def exr_headers(self, files, offsets=None, lengths=None, chan_cap=32):
        """The attribute lists of a batch of OpenEXR files -> ExrBatch.  files: a list of bytes objects or uint8 tensors (concatenated
        and uploaded where they are not on the device), one bytes object, or one uint8 device tensor with offsets / lengths (int64 /
        int32 tables, file i = data[offsets[i] : + lengths[i]]; neither: the tensor is ONE file).  chan_cap: channels listed per
        file.  No synchronisation; a file the call flags (XE_*) is listed and raises nothing."""
        host = None
        if isinstance(files, (list, tuple)):
            import numpy as np
            sizes = [int(b.numel()) if isinstance(b, torch.Tensor) else len(b) for b in files]
            offs = np.zeros(len(files), dtype=np.int64)
            if len(files) > 1:
                np.cumsum(sizes[:-1], out=offs[1:])
            offsets, lengths = torch.from_numpy(offs), torch.tensor(sizes, dtype=torch.int32)
            if files and all(isinstance(b, torch.Tensor) for b in files):
                files = torch.cat([b.to(self.device).reshape(-1) for b in files]).contiguous()
            else:
                files = host = b"".join(bytes(b.cpu().numpy().tobytes()) if isinstance(b, torch.Tensor) else bytes(b) for b in files)
        elif isinstance(files, (bytes, bytearray, memoryview)):
            host = bytes(files)
        data = self._zip_data(files)
        if offsets is None:
            offsets = torch.zeros(1, dtype=torch.int64)
            lengths = torch.tensor([int(data.numel())], dtype=torch.int32)
        offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
        lengths = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        n, chan_cap = int(lengths.numel()), int(chan_cap)
        if int(offsets.numel()) < n:
            raise ValueError("exr_headers: %d lengths need %d offsets" % (n, n))
        if chan_cap < 1:
            raise ValueError("exr_headers: chan_cap must be at least 1")
        images = torch.zeros((n, EXR_IMAGE_BYTES), dtype=torch.uint8, device=self.device)
        chans = torch.zeros((n, chan_cap, EXR_CHANNEL_BYTES), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.zmi_exr_headers_dev(self._ctx, data.data_ptr() if data.numel() else None, offsets.data_ptr() if n else None,
                                              lengths.data_ptr() if n else None, n, images.data_ptr() if n else None,
                                              chans.data_ptr() if n else None, chan_cap, _stream_ptr()), "zmi_exr_headers_dev")
        return ExrBatch(data, offsets, lengths, images, chans, chan_cap, host)

    def exr_read(self, batch, sel=None, align=16, out=None):
        """Files of an ExrBatch, inflated, unzipped and cut into channel planes, densely in one buffer -> (out, out_off int64 [n_sel +
        1], out_len int32 [n_sel], status int32 [n_sel]).  Slot j stands at out[out_off[j] : out_off[j] + out_len[j]]: the channels'
        [H, W] planes in list order (ExrBatch.image / ExrBatch.channel give the views); out_off[-1] is the room the selection needs.
        sel (a list or an int32 tensor) selects, None: every file.  status 0: every check passed; every other status has length 0 and
        nothing is raised for a file.  last_exr_detail keeps the XE_* tensor.  The bounds the call needs -- chunks, raw bytes, room --
        come from the host copy of the batch's tables (one synchronisation the first time the batch is used)."""
        b = batch
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        if out is not None and (out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError("exr_read: out must be a contiguous uint8 tensor on %s" % (self.device,))
        n = b.n
        picks = list(range(n)) if sel is None else [int(k) for k in (sel.tolist() if isinstance(sel, torch.Tensor) else sel)]
        d_sel = None
        if sel is not None:
            d_sel = (sel if isinstance(sel, torch.Tensor) else torch.tensor(picks, dtype=torch.int64)).to(device=self.device, dtype=torch.int32).contiguous()
        n_sel = len(picks)
        rec = b._tables()[0] if n else None
        chunks = decoded = room = 0
        for k in picks:
            if 0 <= k < n and int(rec[k]["status"]) == 0:
                chunks += int(rec[k]["n_chunks"])
                decoded += int(rec[k]["height"]) * int(rec[k]["row_bytes"])
                room += -(-int(rec[k]["region_bytes"]) // align) * align
        out_off = torch.zeros(n_sel + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        status = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        detail = torch.zeros(n_sel, dtype=torch.int32, device=self.device)
        self.last_exr_detail = detail
        if out is None:
            out = torch.empty(room, dtype=torch.uint8, device=self.device)
        _lib.check(self.L.zmi_exr_read_dev(self._ctx, b.data.data_ptr() if n else None, b.offsets.data_ptr() if n else None,
                                           b.lengths.data_ptr() if n else None, b.images.data_ptr() if n else None,
                                           b.chans.data_ptr() if n else None, b.chan_cap, n,
                                           d_sel.data_ptr() if d_sel is not None and n_sel else None, n_sel, chunks, decoded, 0, int(align),
                                           out.data_ptr() if out.numel() else None, int(out.numel()), out_off.data_ptr(), out_len.data_ptr(),
                                           status.data_ptr(), detail.data_ptr(), _stream_ptr()), "zmi_exr_read_dev")
        return out, out_off, out_len, status

    # ---- writing PNG images (include/zmi355.h) ----
    _PNG_FILTERS ={"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
    _PNG_COLOUR = {1: 0, 2: 4, 3: 2, 4: 6}

    def png_bound(self, n_images, scan_bytes, piece_bytes=1 << 20, align=1, level=6):
        """room that always suffices for n_images files whose filtered scanlines -- (1 + row_bytes) * height each -- are scan_bytes in all"""
        return int(self.L.zmi_png_bound(int(n_images), int(scan_bytes), int(piece_bytes), int(align), int(level)))

    def png_encode(self, images, level=6, strategy=0, filter="adaptive", piece_bytes=1 << 20, align=1, native16=True, out=None,
                   scan_bytes=None):
        """A batch of images as complete PNG files, one behind the other in one buffer -> (out, out_off int64 [n + 1], out_len int32
        [n], status int32 [n]), as png_decode returns them: file i is out[out_off[i] : out_off[i] + out_len[i]], out_off[-1] the room
        the batch needs.  images: a list of device tensors [H, W] or [H, W, C] with C 1 .. 4 (gray, gray + alpha, RGB, RGBA) of dtype
        uint8 (depth 8) or uint16 / int16 (depth 16, the 16 bits as they stand), joined by ONE torch.cat; or the tuple (data, offsets,
        lengths, table) of a uint8 device buffer, the int64 / int32 tables of the images' places in it and their records (a uint8
        [n, 48] tensor or a PngBatch, of which width, height, depth and colour are read): packed depths, and what png_decode returned --
        png_encode((data, out_off, out_len, batch)) writes a decoded batch again.  filter: "adaptive" (per row, the least sum of absolute
        differences), "none", "sub", "up", "average", "paeth", or 0 .. 5.  native16: 16-bit samples stand little-endian in the buffer.
        scan_bytes (the tuple form only): the caller's bound on the sum of (1 + row_bytes) * height over the images, which sizes the
        scratch and the piece table; None: twice the buffer, which holds where no two images share bytes of it.  A per-image failure is a
        status with length 0 and raises nothing; data and out are never copied; last_png_written keeps the table zmi_png_headers_dev
        would list for the files.  No synchronisation."""
        if isinstance(filter, str):
            if filter not in self._PNG_FILTERS:
                raise ValueError("png_encode: filter must be one of %s" % ", ".join(sorted(self._PNG_FILTERS)))
            filter = self._PNG_FILTERS[filter]
        if not 0 <= int(filter) <= 5:
            raise ValueError("png_encode: filter must be 0 .. 5")
        if align < 1 or align > 4096 or align & (align - 1):
            raise ValueError("align must be a power of two, 1 .. 4096")
        if out is not None and (out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError("png_encode: out must be a contiguous uint8 tensor on %s" % self.device)
        if isinstance(images, tuple) and len(images) == 4 and isinstance(images[1], torch.Tensor) and images[1].dtype in (torch.int64, torch.int32):
            data, offsets, lengths, table = images                   # (no image has an offset table's dtype)
            if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.device != self.device or not data.is_contiguous():
                raise ValueError("png_encode: data must be a contiguous uint8 tensor on %s" % self.device)
            table = table.images if isinstance(table, PngBatch) else table
            if table.dtype != torch.uint8 or table.device != self.device or table.dim() != 2 or table.shape[1] != PNG_IMAGE_BYTES:
                raise ValueError("png_encode: the table must be a uint8 [n, %d] tensor on %s" % (PNG_IMAGE_BYTES, self.device))
            table = table.contiguous()
            n = int(table.shape[0])
            offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
            lengths = lengths.to(device=self.device, dtype=torch.int32).contiguous()
            if int(offsets.numel()) < n or int(lengths.numel()) < n:
                raise ValueError("png_encode: %d records need %d offsets and lengths" % (n, n))
            # (1 + row_bytes) * height <= 2 * row_bytes * height: the buffer bounds the scanlines without a look at the device
            scan_bytes = 2 * int(data.numel()) if scan_bytes is None else int(scan_bytes)
        else:
            import numpy as np
            if scan_bytes is not None:
                raise ValueError("png_encode: scan_bytes goes with (data, offsets, lengths, table); a list's shapes give it")
            if not isinstance(images, (list, tuple)) or len(images) == 0:
                raise ValueError("png_encode: images must be a non-empty list of tensors or (data, offsets, lengths, table)")
            table = np.zeros((len(images), PNG_IMAGE_BYTES), dtype=np.uint8)
            words, parts, offs, lens, at, scan_bytes = table.view("<u4"), [], [], [], 0, 0
            for k, t in enumerate(images):
                if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype not in (torch.uint8, torch.uint16, torch.int16):
                    raise ValueError("png_encode: image %d must be a uint8, uint16 or int16 tensor on %s" % (k, self.device))
                if t.dim() not in (2, 3) or (t.dim() == 3 and not 1 <= t.shape[2] <= 4) or t.numel() == 0:
                    raise ValueError("png_encode: image %d must be [H, W] or [H, W, C] with C 1 .. 4, not %s" % (k, tuple(t.shape)))
                c = 1 if t.dim() == 2 else int(t.shape[2])
                words[k, 0], words[k, 1] = int(t.shape[1]), int(t.shape[0])
                table[k, 8], table[k, 9] = 8 * t.element_size(), self._PNG_COLOUR[c]
                body = t.contiguous().view(-1).view(torch.uint8)
                parts.append(body)
                offs.append(at)
                lens.append(int(body.numel()))
                at += lens[-1]
                scan_bytes += lens[-1] + int(t.shape[0])
            data = parts[0] if len(parts) == 1 else torch.cat(parts)
            n = len(images)
            offsets = torch.tensor(offs, dtype=torch.int64, device=self.device)
            lengths = torch.tensor(lens, dtype=torch.int32, device=self.device)
            table = torch.from_numpy(table).to(self.device)
        if out is None:
            out = torch.empty(self.png_bound(n, scan_bytes, piece_bytes, align, level), dtype=torch.uint8, device=self.device)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.last_png_written = written = torch.zeros((n, PNG_IMAGE_BYTES), dtype=torch.uint8, device=self.device)
        _lib.check(self.L.zmi_png_encode_dev(self._ctx, data.data_ptr() if data.numel() else None, offsets.data_ptr() if n else None,
                                             lengths.data_ptr() if n else None, table.data_ptr() if n else None, n, int(scan_bytes),
                                             PNG_NATIVE16 if native16 else 0, int(filter), int(piece_bytes), int(level), int(strategy), int(align),
                                             out.data_ptr() if out.numel() else None, int(out.numel()), out_off.data_ptr(),
                                             out_len.data_ptr() if n else None, written.data_ptr() if n else None,
                                             status.data_ptr() if n else None, _stream_ptr()), "zmi_png_encode_dev")
        return out, out_off, out_len, status

    def save_png(self, tensor, **kw):
        """One image ([H, W] or [H, W, C], uint8 / uint16 / int16, on the device) -> the bytes of its .png file; a status that is not 0
        raises.  Keywords as png_encode's."""
        out, off, ln, st = self.png_encode([tensor], **kw)
        host = torch.stack([ln.to(torch.int64), st.to(torch.int64)]).view(-1).tolist()
        if host[1] != 0:
            raise RuntimeError("zmi_png_encode_dev: status %d" % host[1])
        return out[:host[0]].cpu().numpy().tobytes()

    # ---- writing TIFF files (include/zmi355.h) ----
    _TIFF_DTYPES = {torch.uint8: (8, 1), torch.int8: (8, 2), torch.uint16: (16, 1), torch.int16: (16, 2), torch.float16: (16, 3),
                    torch.uint32: (32, 1), torch.int32: (32, 2), torch.float32: (32, 3), torch.uint64: (64, 1), torch.int64: (64, 2),
                    torch.float64: (64, 3)}

    def _tiff_desc(self, shape, dtype, tile, rows_per_strip, predictor, level, strategy, piece_bytes, align, bigtiff, photometric, extra_samples,
                   assemble):
        """the zmi_tiff_write of a page of `shape` = (H, W, C) and a torch dtype -- those TiffFile.dtype returns"""
        if dtype not in self._TIFF_DTYPES:
            raise ValueError("tiff_write: dtype %s is not one a TIFF sample has" % (dtype,))
        bits, fmt = self._TIFF_DTYPES[dtype]
        h, w, c = (int(v) for v in shape)
        if predictor == "auto":
            predictor = 3 if fmt == 3 else 2
        if photometric is None:
            photometric = 2 if c - int(extra_samples) >= 3 else 1
        tw, th = (0, 0) if tile is None else ((int(tile), int(tile)) if isinstance(tile, int) else (int(tile[0]), int(tile[1])))
        flags = (TIFF_ASSEMBLE if assemble else 0) | (TIFF_BIGTIFF if bigtiff else 0)
        return _lib.TiffWrite(w, h, tw, th, int(rows_per_strip or 0), bits, c, fmt, int(predictor), int(photometric), int(extra_samples),
                              2 if extra_samples else 0, flags, int(piece_bytes), int(align), int(level), int(strategy))

    def tiff_bound(self, shape, dtype, tile=None, rows_per_strip=None, predictor="auto", level=6, strategy=0, piece_bytes=1 << 20, align=16,
                   bigtiff=False, photometric=None, extra_samples=0):
        """room that always suffices for the file of a page of shape (H, W, C) and that dtype; keywords as tiff_write's"""
        import ctypes as C
        d = self._tiff_desc(shape, dtype, tile, rows_per_strip, predictor, level, strategy, piece_bytes, align, bigtiff, photometric,
                            extra_samples, True)
        bound = int(self.L.zmi_tiff_bound(C.byref(d)))
        if bound == 0:
            raise ValueError("tiff_bound: these arguments describe no page zmi_tiff_write_dev writes")
        return bound

    def tiff_write(self, image_or_segments, tile=None, rows_per_strip=None, predictor="auto", level=6, strategy=0, piece_bytes=1 << 20, align=16,
                   bigtiff=False, photometric=None, extra_samples=0, out=None):
        """One page as a complete little-endian Deflate TIFF file in device memory -> (out, file_len int64 [1], seg_len int32 [n_segs],
        status int32 [n_segs + 1]): the file is out[:file_len], file_len the room it needs whether or not it fitted, seg_len the byte
        counts of its strips or tiles, status[k] segment k's and status[-1] the file's (Z_BUF_ERROR: out is too small).  A device
        tensor [H, W] or [H, W, C], C 1 .. 8, of a dtype TiffFile.dtype returns is the page as one image: the predict kernel cuts the
        segments and pads edge tiles with zeros.  The tuple (data, offsets, shape, dtype) is the dense form: segment k is the bytes
        data[offsets[k]:] as tiff_read(assemble=False) returns them ([rows, seg_w, C], edge tiles with their padding as it stands),
        shape = (H, W, C).  tile: None for strips of rows_per_strip rows (None: one strip), an int or (tile_w, tile_h), multiples of
        16.  predictor: 1, 2, 3 or "auto" -- 3 for floating dtypes, 2 otherwise.  align: where every segment starts in the file;
        extra_samples: how many of the C samples are unassociated alpha (tag 338); photometric None: RGB for 3 colour samples and
        more, BlackIsZero otherwise.  last_tiff_written keeps the record tiff_directory would list for the file.  No synchronisation."""
        import ctypes as C
        if isinstance(image_or_segments, torch.Tensor):
            t = image_or_segments
            if t.device != self.device or t.dim() not in (2, 3) or t.numel() == 0:
                raise ValueError("tiff_write: the image must be a [H, W] or [H, W, C] tensor on %s" % (self.device,))
            shape, dtype = (int(t.shape[0]), int(t.shape[1]), 1 if t.dim() == 2 else int(t.shape[2])), t.dtype
            data, offsets, assemble = t.contiguous().view(-1).view(torch.uint8), None, True
        else:
            data, offsets, shape, dtype = image_or_segments
            if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.device != self.device or not data.is_contiguous():
                raise ValueError("tiff_write: data must be a contiguous uint8 tensor on %s" % (self.device,))
            offsets, assemble = offsets.to(device=self.device, dtype=torch.int64).contiguous(), False
        if out is not None and (out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError("tiff_write: out must be a contiguous uint8 tensor on %s" % (self.device,))
        d = self._tiff_desc(shape, dtype, tile, rows_per_strip, predictor, level, strategy, piece_bytes, align, bigtiff, photometric,
                            extra_samples, assemble)
        bound = int(self.L.zmi_tiff_bound(C.byref(d)))
        if bound == 0:
            raise ValueError("tiff_write: these arguments describe no page zmi_tiff_write_dev writes")
        seg_w, seg_h = (d.tile_w, d.tile_h) if d.tile_w else (d.width, d.rows_per_strip if 0 < d.rows_per_strip < d.height else d.height)
        n = -(-d.width // seg_w) * -(-d.height // seg_h)
        if offsets is not None and int(offsets.numel()) < n:
            raise ValueError("tiff_write: %d segments need %d offsets" % (n, n))
        if out is None:
            out = torch.empty(bound, dtype=torch.uint8, device=self.device)
        file_len = torch.zeros(1, dtype=torch.int64, device=self.device)
        seg_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n + 1, dtype=torch.int32, device=self.device)     # the segments' | the file's
        self.last_tiff_written = written = torch.zeros(TIFF_PAGE_BYTES, dtype=torch.uint8, device=self.device)
        _lib.check(self.L.zmi_tiff_write_dev(self._ctx, C.byref(d), data.data_ptr(), offsets.data_ptr() if offsets is not None else None,
                                             out.data_ptr() if out.numel() else None, int(out.numel()), file_len.data_ptr(), seg_len.data_ptr(),
                                             status.data_ptr(), status.data_ptr() + 4 * n, written.data_ptr(), _stream_ptr()),
                   "zmi_tiff_write_dev")
        return out, file_len, seg_len, status

    def save_tiff(self, tensor, **kw):
        """One image ([H, W] or [H, W, C] on the device) -> the bytes of its .tif file; a status that is not 0 raises.  Keywords as
        tiff_write's."""
        out, file_len, seg_len, status = self.tiff_write(tensor, **kw)
        host = torch.cat([file_len, status[-1:].to(torch.int64)]).tolist()
        if host[1] != 0:
            raise RuntimeError("zmi_tiff_write_dev: status %d" % host[1])
        return out[:host[0]].cpu().numpy().tobytes()

    # ---- writing OpenEXR images (include/zmi355.h) ----
    _EXR_TYPES = {torch.int32: 0, torch.float16: 1, torch.float32: 2}
    _EXR_COMPRESSION = {"none": 0, "zips": 2, "zip": 3, "pxr24": 5}

    def _exr_desc(self, shape, channels, compression, tile, origin, display_window, level, strategy, piece_bytes, align):
        """the zmi_exr_write of images of `shape` = (H, W) and channels [(name, torch dtype)] sorted by name -> (the struct, what keeps
        its channel array alive)"""
        import ctypes
        h, w = (int(v) for v in shape)
        if compression not in self._EXR_COMPRESSION:
            raise ValueError("exr_write: compression must be 'zip', 'zips', 'pxr24' or 'none'")
        for _, dt in channels:
            if dt not in self._EXR_TYPES:
                raise ValueError("exr_write: dtype %s is not one an OpenEXR channel has (float16, float32, int32)" % (dt,))
        arr = (_lib.ExrWriteChannel * max(1, len(channels)))(*[_lib.ExrWriteChannel(n.encode("latin-1"), self._EXR_TYPES[dt]) for n, dt in channels])
        x0, y0 = (int(v) for v in origin)
        dw = (x0, y0, x0 + w - 1, y0 + h - 1)
        disp = tuple(int(v) for v in display_window) if display_window is not None else (0, 0, w - 1, h - 1)
        tw, th = (0, 0) if tile is None else ((int(tile), int(tile)) if isinstance(tile, int) else (int(tile[0]), int(tile[1])))
        d = _lib.ExrWrite((ctypes.c_int32 * 4)(*dw), (ctypes.c_int32 * 4)(*disp), len(channels), arr, self._EXR_COMPRESSION[compression], tw, th,
                          0, int(piece_bytes), int(align), int(level), int(strategy))
        return d, arr

    def exr_bound(self, shape, channels, n_images=1, compression="zip", tile=None, origin=(0, 0), display_window=None, level=6, strategy=0,
                  piece_bytes=1 << 20, align=16):
        """the room n_images files of images of shape (H, W) need at most; channels: [(name, torch dtype)]; keywords as exr_write's"""
        import ctypes
        d, keep = self._exr_desc(shape, sorted(channels, key=lambda c: c[0].encode("latin-1")), compression, tile, origin, display_window, level, strategy, piece_bytes, align)
        bound = int(self.L.zmi_exr_bound(ctypes.byref(d), int(n_images)))
        if bound == 0:
            raise ValueError("exr_bound: these arguments describe no image zmi_exr_write_dev writes")
        return bound

    def exr_write(self, images, channels=None, compression="zip", tile=None, origin=(0, 0), display_window=None, level=6, strategy=0,
                  piece_bytes=1 << 20, align=16, out=None):
        """A batch of images of ONE layout as complete OpenEXR files in one device buffer -> (out, out_off int64 [n + 1], out_len int32
        [n], status int32 [n]): file i is out[out_off[i] : out_off[i] + out_len[i]], out_off[-1] the room the batch needs whether or
        not it fitted (Z_BUF_ERROR with length 0 where out is too small).  images: a [N, C, H, W] or [C, H, W] device tensor of
        float16, float32 or int32 (UINT bits) with `channels` = the C names; or a dict, or a list of dicts, name -> [H, W] tensor, of
        mixed dtypes.  The names are sorted here, as the file wants them, and the planes laid out as exr_read returns them; every
        image must have the layout of the first.  compression "zip" (16 scanlines a chunk), "zips" (one), "pxr24" (16; float32 channels
        keep 24 bits in the chunks that shrink, every other value is exact) or "none"; tile: None for scanlines, an int or (tile_w, tile_h); origin: (xMin, yMin) of the data window; display_window None: (0, 0, W - 1, H - 1).
        last_exr_written keeps the records exr_headers would list for the files, last_exr_chunk_len every chunk's dataSize (== the
        chunk's raw size where it was stored raw).  No synchronisation."""
        import ctypes
        dense = None
        if isinstance(images, torch.Tensor):
            t = images if images.dim() == 4 else images.unsqueeze(0)
            if t.dim() != 4 or t.device != self.device or t.numel() == 0:
                raise ValueError("exr_write: a tensor must be [N, C, H, W] or [C, H, W] on %s" % (self.device,))
            if channels is None or len(channels) != t.shape[1]:
                raise ValueError("exr_write: a tensor needs `channels`, one name per plane")
            names = [str(nm) for nm in channels]
            if len(set(names)) != len(names):
                raise ValueError("exr_write: a channel name stands twice")
            plane = int(t.shape[2]) * int(t.shape[3]) * t.element_size()
            if t.is_contiguous() and plane % 4 == 0 and names == sorted(names, key=lambda s: s.encode("latin-1")):
                dense = t                                                    # the tensor IS the regions, one behind the other: no copy
            images = [{nm: t[i, c] for c, nm in enumerate(names)} for i in range(t.shape[0])]
        elif isinstance(images, dict):
            images = [images]
        if not images or not images[0]:
            raise ValueError("exr_write: no image, or no channel")
        names = sorted(images[0], key=lambda s: s.encode("latin-1"))
        layout = [(nm, images[0][nm].dtype) for nm in names]
        h, w = (int(v) for v in images[0][names[0]].shape)
        parts, offs, at = [], [], 0
        if dense is not None:
            parts, offs = [dense.view(-1).view(torch.uint8)], [i * len(names) * plane for i in range(len(images))]
        for im in ([] if dense is not None else images):
            if sorted(im, key=lambda s: s.encode("latin-1")) != names:
                raise ValueError("exr_write: every image must have the channels of the first")
            offs.append(at)
            for nm, dt in layout:
                p = im[nm]
                if p.dtype != dt or tuple(p.shape) != (h, w) or p.device != self.device:
                    raise ValueError("exr_write: channel %r differs from the first image's in dtype, shape or device" % nm)
                pad = -at % 4
                if pad:
                    parts.append(torch.zeros(pad, dtype=torch.uint8, device=self.device))
                    at += pad
                parts.append(p.contiguous().view(-1).view(torch.uint8))
                at += int(parts[-1].numel())
            pad = -at % 4                                                     # the next image's first plane starts at a multiple of 4
            if pad:
                parts.append(torch.zeros(pad, dtype=torch.uint8, device=self.device))
                at += pad
        data = torch.cat(parts) if len(parts) > 1 else parts[0]
        if out is not None and (out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()):
            raise ValueError("exr_write: out must be a contiguous uint8 tensor on %s" % (self.device,))
        d, keep = self._exr_desc((h, w), layout, compression, tile, origin, display_window, level, strategy, piece_bytes, align)
        n = len(images)
        bound = int(self.L.zmi_exr_bound(ctypes.byref(d), n))
        if bound == 0:
            raise ValueError("exr_write: these arguments describe no image zmi_exr_write_dev writes")
        tw, th = (d.tile_w, d.tile_h) if d.tile_w else (w, 16 if d.compression in (3, 5) else 1)
        nc = -(-w // tw) * -(-h // th)
        if out is None:
            out = torch.empty(bound, dtype=torch.uint8, device=self.device)
        in_off = torch.tensor(offs, dtype=torch.int64).to(self.device)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        chunk_len = torch.zeros((n, nc), dtype=torch.int32, device=self.device)
        written = torch.zeros((n, EXR_IMAGE_BYTES), dtype=torch.uint8, device=self.device)
        wch = torch.zeros((n, len(layout), EXR_CHANNEL_BYTES), dtype=torch.uint8, device=self.device)
        self.last_exr_written, self.last_exr_chunk_len = (written, wch), chunk_len
        _lib.check(self.L.zmi_exr_write_dev(self._ctx, ctypes.byref(d), data.data_ptr(), in_off.data_ptr(), n,
                                            out.data_ptr() if out.numel() else None, int(out.numel()), out_off.data_ptr(), out_len.data_ptr(),
                                            chunk_len.data_ptr(), written.data_ptr(), wch.data_ptr(), status.data_ptr(), _stream_ptr()),
                   "zmi_exr_write_dev")
        return out, out_off, out_len, status

    def save_exr(self, image, **kw):
        """One image (a [C, H, W] tensor with channels=..., or a dict name -> [H, W] tensor) -> the bytes of its .exr file; a status
        that is not 0 raises.  Keywords as exr_write's."""
        out, out_off, out_len, status = self.exr_write(image, **kw)
        if int(status.numel()) != 1:
            raise ValueError("save_exr: one image")
        host = torch.cat([out_len.to(torch.int64), status.to(torch.int64)]).tolist()
        if host[1] != 0:
            raise RuntimeError("zmi_exr_write_dev: status %d" % host[1])
        return out[:host[0]].cpu().numpy().tobytes()

    # ---- writing ZIP archives (include/zmi355.h) ----
    def zip_bound(self, n_entries, names_bytes, in_bytes, piece_bytes=1 << 20, level=6):
        return int(self.L.zmi_zip_bound(int(n_entries), int(names_bytes), int(in_bytes), int(piece_bytes), int(level)))

    def _zip_names(self, names):
        """list of str (encoded as UTF-8) or (blob uint8, offsets int64 [n + 1]) -> the pair on the device and the blob's size"""
        if isinstance(names, (tuple, list)) and len(names) == 2 and isinstance(names[0], torch.Tensor):
            blob, off = names
            blob = blob.to(device=self.device, dtype=torch.uint8).contiguous().view(-1)
            return blob, off.to(device=self.device, dtype=torch.int64).contiguous(), int(blob.numel())
        import numpy as np
        enc = [nm.encode("utf-8") if isinstance(nm, str) else bytes(nm) for nm in names]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in enc], out=off[1:])
        blob = torch.from_numpy(np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8).copy()).to(self.device)
        return blob, torch.from_numpy(off).to(self.device), int(off[-1])

    def zip_write(self, data, offsets, lengths, names, level=6, strategy=0, piece_bytes=1 << 20, base=0, dos_time=None, ext_attr=None,
                  directory=False, out=None):
        """The entries data[offsets[i] : + lengths[i]] (uint8 device tensor, int64 / int32 tables) as a ZIP archive -> a uint8 view of
        exactly the archive, and with directory=True also its ZipDirectory, made from the writer's own table and info: names(), index()
        and zip_read work on it without parsing anything again.  names: a list of str, or a (blob, offsets) pair of tensors.  level 0
        stores; dos_time / ext_attr: int32 tensors, one word per entry (None: 1980-01-01 and a regular file, 0644).  base: the file
        position the archive will stand at.  One synchronisation, for the length; a non-zero status raises.  Tables and the names blob
        on another device, of another integer type or not contiguous are converted; data must be a contiguous uint8 tensor on the
        engine's device (it is never copied), as must out."""
        for what, t in (("data", data), ("out", out)):
            if t is not None and (t.dtype != torch.uint8 or t.device != self.device or not t.is_contiguous()):
                raise ValueError("zip_write: %s must be a contiguous uint8 tensor on %s" % (what, self.device))
        offsets = offsets.to(device=self.device, dtype=torch.int64).contiguous()
        lengths = lengths.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(lengths.numel())
        if int(offsets.numel()) < n:
            raise ValueError("zip_write: %d lengths need %d offsets" % (n, n))
        blob, name_off, names_bytes = self._zip_names(names)
        if int(name_off.numel()) != n + 1:
            raise ValueError("names: %d entries need %d offsets" % (n, n + 1))
        in_bytes = int(data.numel())
        if out is None:
            out = torch.empty(self.zip_bound(n, names_bytes, in_bytes, piece_bytes, level), dtype=torch.uint8, device=self.device)
        meta = torch.zeros(8, dtype=torch.int64, device=self.device)     # length | status (int32) | zmi_zip_info
        entries = torch.empty((n, ZIP_ENTRY_BYTES), dtype=torch.uint8, device=self.device) if directory else None
        words = [None if t is None else t.to(device=self.device, dtype=torch.int32).contiguous() for t in (dos_time, ext_attr)]
        _lib.check(self.L.zmi_zip_write_dev(self._ctx, data.data_ptr() if in_bytes else None, offsets.data_ptr() if n else None,
                                            lengths.data_ptr() if n else None, n, in_bytes, blob.data_ptr(), name_off.data_ptr(),
                                            words[0].data_ptr() if words[0] is not None and n else None,
                                            words[1].data_ptr() if words[1] is not None and n else None, int(piece_bytes), int(level),
                                            int(strategy), int(base), out.data_ptr() if out.numel() else None, int(out.numel()), meta.data_ptr(),
                                            entries.data_ptr() if directory and n else None, meta.data_ptr() + 16 if directory else None,
                                            meta.data_ptr() + 8, _stream_ptr()), "zmi_zip_write_dev")
        host = meta.tolist()
        length, st = host[0], host[1] & 0xFFFFFFFF
        status = st - (1 << 32) if st >= 1 << 31 else st
        if status != 0:
            raise RuntimeError("zmi_zip_write_dev: status %d (archive of %d bytes, room for %d)" % (status, length, out.numel()))
        if not directory:
            return out[:length]
        info = {"n_entries": host[2], "n_listed": host[3], "cd_off": host[4], "cd_size": host[5], "base": host[6], "status": 0, "detail": 0}
        return out[:length], ZipDirectory(out[:length], entries, info)

    _NPY_DESCR = {torch.bool: "|b1", torch.uint8: "|u1", torch.int8: "|i1", torch.int16: "<i2", torch.int32: "<i4", torch.int64: "<i8",
                  torch.float16: "<f2", torch.float32: "<f4", torch.float64: "<f8"}

    def save_npz(self, arrays, level=6, piece_bytes=1 << 20):
        """arrays: dict of name -> device tensor -> the bytes of an .npz numpy.load opens (level 0: what numpy.savez writes, stored;
        otherwise savez_compressed's layout).  The version-1.0 .npy headers are made on the host, padded to 64 bytes; headers and
        payloads become one buffer with one torch.cat and one archive with one zip_write.  dtypes: those with a NumPy twin (bool, uint8,
        int8, int16, int32, int64, float16, float32, float64); any other, bfloat16 included, is a TypeError."""
        import numpy as np
        parts, offs, lens, names, at = [], [], [], [], 0
        for name, t in arrays.items():
            if t.dtype not in self._NPY_DESCR:
                raise TypeError("save_npz: %r has dtype %s, which has no NumPy twin" % (name, t.dtype))
            shape = "(%d,)" % t.shape[0] if t.dim() == 1 else "(%s)" % ", ".join("%d" % d for d in t.shape)
            head = "{'descr': '%s', 'fortran_order': False, 'shape': %s, }" % (self._NPY_DESCR[t.dtype], shape)
            head += " " * (-(10 + len(head) + 1) % 64) + "\n"
            head = b"\x93NUMPY\x01\x00" + len(head).to_bytes(2, "little") + head.encode("latin1")
            body = t.to(self.device).contiguous().view(-1)
            body = body.view(torch.uint8) if body.numel() else torch.empty(0, dtype=torch.uint8, device=self.device)
            parts += [torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).to(self.device), body]
            offs.append(at)
            lens.append(len(head) + int(body.numel()))
            names.append(name + ".npy")
            at += lens[-1]
        data = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device=self.device)
        out = self.zip_write(data, torch.tensor(offs, dtype=torch.int64, device=self.device),
                             torch.tensor(lens, dtype=torch.int32, device=self.device), names, level=level, piece_bytes=piece_bytes)
        return out.cpu().numpy().tobytes()

    # ---- checksums ----
    def checksums(self, data, offsets, lengths, adler=True, crc=True, out_adler=None, out_crc=None):
        """(adler int32 [n], crc int32 [n]); the array of a checksum that was not asked for is left as it is (zeros when
        allocated here)"""
        n = int(lengths.numel())
        a = torch.zeros(n, dtype=torch.int32, device=self.device) if out_adler is None else out_adler
        c = torch.zeros(n, dtype=torch.int32, device=self.device) if out_crc is None else out_crc
        kind = (1 if adler else 0) | (2 if crc else 0)
        _lib.check(self.L.zmi_checksum_batch_dev(self._ctx, data.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, kind,
                                                 a.data_ptr(), c.data_ptr(), _stream_ptr()), "zmi_checksum_batch_dev")
        return a, c


def _check_zdict(zdict, device):
    if zdict.dtype != torch.uint8 or zdict.device != device or not zdict.is_contiguous():
        raise ValueError("zdict must be a contiguous uint8 tensor on %s" % (device,))


def _len_status(meta):
    """int64 [2] device words (length, int32 status in the low half of the second) -> host ints, one synchronisation"""
    length, st = meta.tolist()
    st &= 0xFFFFFFFF
    return int(length), st - (1 << 32) if st >= 1 << 31 else st


def uniform_layout(n, shard_bytes, device):
    """offsets/lengths tensors for n back-to-back shards of equal size"""
    off = (torch.arange(n, dtype=torch.int64, device=device) * shard_bytes)
    ln = torch.full((n,), shard_bytes, dtype=torch.int32, device=device)
    return off, ln
