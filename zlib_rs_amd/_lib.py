"""ctypes binding of libzmi355.so (the C ABI in include/zmi355.h).  Fails loudly when the HIP
library is missing -- there is no CPU fallback in this package."""
import ctypes as C
import os

from ._build import LIB

_lib = None


class TiffWrite(C.Structure):
    """zmi_tiff_write (include/zmi355.h): host memory, read during zmi_tiff_bound / zmi_tiff_write_dev"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("rows_per_strip", C.c_uint32),
                ("bits", C.c_uint16), ("samples", C.c_uint16), ("sample_format", C.c_uint16), ("predictor", C.c_uint16),
                ("photometric", C.c_uint16), ("extra_samples", C.c_uint16), ("extra_kind", C.c_uint16), ("flags", C.c_uint32),
                ("piece_bytes", C.c_uint32), ("out_align", C.c_uint32), ("level", C.c_int32), ("strategy", C.c_int32)]


class ExrWriteChannel(C.Structure):
    """zmi_exr_write_channel (include/zmi355.h)"""
    _fields_ = [("name", C.c_char_p), ("pixel_type", C.c_int32)]


class ExrWrite(C.Structure):
    """zmi_exr_write (include/zmi355.h): host memory, read during zmi_exr_bound / zmi_exr_write_dev"""
    _fields_ = [("data_window", C.c_int32 * 4), ("display_window", C.c_int32 * 4), ("n_channels", C.c_uint32),
                ("channels", C.POINTER(ExrWriteChannel)), ("compression", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("flags", C.c_uint32), ("piece_bytes", C.c_uint32), ("out_align", C.c_uint32), ("level", C.c_int32), ("strategy", C.c_int32)]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(this package has no CPU fallback)" % LIB)
    L = C.CDLL(LIB)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.zmi_version.restype = C.c_char_p
    L.zmi_last_error.restype = C.c_char_p
    L.zmi_ctx_create.argtypes = [C.POINTER(vp), i32]
    L.zmi_ctx_destroy.argtypes = [vp]
    L.zmi_ctx_set_scratch_limit.argtypes = [vp, u64]
    L.zmi_ctx_set_inflate_out_limit.argtypes = [vp, u64]
    L.zmi_deflate_bound.restype = u64
    L.zmi_deflate_bound.argtypes = [u64, i32]
    L.zmi_deflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, vp, u64, vp, vp, vp]
    L.zmi_inflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp, vp]
    # one shared preset dictionary for a whole batch (csrc/lz77.hip, inflate.hip, zmi_api.hip)
    L.zmi_deflate_dict_bound.restype = u64
    L.zmi_deflate_dict_bound.argtypes = [u64, i32]
    L.zmi_deflate_batch_shared_dict_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, vp, u32, vp, u64, vp, vp, vp]
    L.zmi_inflate_batch_shared_dict_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    # batch inflate without an output size table: the size pass, and the dense decode built on it (csrc/inflate.hip, zmi_api.hip)
    L.zmi_inflate_sizes_dev.argtypes = [vp, vp, vp, vp, u32, i32, u32, u32, vp, vp, vp, vp, vp]
    L.zmi_inflate_batch_packed_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp, vp]
    L.zmi_checksum_batch_dev.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp]
    L.zmi_gen_shards_dev.argtypes = [vp, vp, u64, u32, u32, u32, vp]
    L.zmi_gen_shards_strided_dev.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp]
    L.zmi_scan_sizes_dev.argtypes = [vp, vp, u32, vp, vp]
    L.zmi_copy_ranges_dev.argtypes = [vp, vp, vp, u64, vp, u32, u32, vp, vp, u64, vp]
    L.zmi_pack_slab_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp]
    L.zmi_deflate_batch.argtypes = [vp, vp, vp, vp, u32, i32, i32, i32, vp, u64, vp, vp]
    L.zmi_inflate_batch.argtypes = [vp, vp, vp, vp, u32, i32, vp, vp, vp, vp, vp]
    # single-stream deflate (csrc/zmi_api.hip, checksum.hip, pack.hip)
    L.zmi_deflate_stream_bound.restype = u64
    L.zmi_deflate_stream_bound.argtypes = [u64, u32, i32]
    L.zmi_stream_header_bytes.restype = u32
    L.zmi_stream_header_bytes.argtypes = [i32]
    L.zmi_deflate_pieces_stride.restype = u64
    L.zmi_deflate_pieces_stride.argtypes = [u32]
    L.zmi_deflate_stream_dev.argtypes = [vp, vp, u64, u32, i32, i32, i32, u32, vp, u64, vp, vp, vp, vp]
    L.zmi_deflate_pieces_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, i32, u32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_checksum_combine_dev.argtypes = [vp, i32, vp, vp, u32, u32, vp, vp, vp]
    L.zmi_stream_frame_dev.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, u64, vp, vp, vp]
    # single-stream inflate (csrc/inflate.hip, zmi_api.hip)
    L.zmi_inflate_stream_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    L.zmi_stream_find_cuts_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    # ... of streams without flush points: cuts at bit positions, proposed by the block scan (csrc/blockscan.hip)
    L.zmi_stream_find_blocks_dev.argtypes = [vp, vp, u64, i32, u64, vp, u32, vp, vp]
    L.zmi_inflate_stream_bits_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    # random access into one stream: the index kept while it is decoded, byte ranges read from it (csrc/inflate.hip, zmi_api.hip)
    L.zmi_inflate_stream_index_dev.argtypes = [vp, vp, u64, i32, vp, u32, u32, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, u32, vp, vp, vp]
    L.zmi_inflate_ranges_dev.argtypes = [vp, vp, u64, vp, vp, vp, u32, u64, vp, vp, u32, u32, vp, vp, u64, vp, vp, vp]
    # multi-member gzip files: proposals of member starts, then every member decoded in place and verified
    L.zmi_gzip_find_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_inflate_members_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    # writing BGZF: blocked gzip with a block index (csrc/pack.hip, zmi_api.hip)
    L.zmi_bgzf_bound.restype = u64
    L.zmi_bgzf_bound.argtypes = [u64, u32]
    L.zmi_bgzf_blocks_dev.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, vp, u64, vp, vp, vp, vp]
    L.zmi_bgzf_deflate_dev.argtypes = [vp, vp, u64, u32, i32, i32, vp, u64, vp, vp, vp, vp]
    # reading ZIP archives: the directory, then a batch inflate of entries checked against it (csrc/pack.hip, zmi_api.hip)
    L.zmi_zip_walk_tile.restype = u32
    L.zmi_zip_walk_tile.argtypes = []
    L.zmi_zip_directory_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_zip_inflate_dev.argtypes = [vp, vp, u64, vp, u32, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    # reading PNG images: the chunk chain, a batch inflate of the IDAT streams, the scanline unfilter (csrc/png_kernels.h, zmi_api.hip)
    L.zmi_png_strip.restype = u32
    L.zmi_png_strip.argtypes = []
    L.zmi_png_headers_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.zmi_png_decode_dev.argtypes = [vp, vp, vp, vp, vp, u32, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    # writing ZIP archives: entries, directory, ZIP64 (csrc/pack.hip, checksum.hip, zmi_api.hip)
    L.zmi_zip_bound.restype = u64
    L.zmi_zip_bound.argtypes = [u32, u64, u64, u32, i32]
    L.zmi_zip_write_dev.argtypes = [vp, vp, vp, vp, u32, u64, vp, vp, vp, vp, u32, i32, i32, u64, vp, u64, vp, vp, vp, vp, vp]
    # writing PNG images: the forward filter, deflate in pieces, the chunks (csrc/png_kernels.h, checksum.hip, zmi_api.hip)
    L.zmi_png_filter_tile.restype = u32
    L.zmi_png_filter_tile.argtypes = []
    L.zmi_png_bound.restype = u64
    L.zmi_png_bound.argtypes = [u32, u64, u32, u32, i32]
    L.zmi_png_encode_dev.argtypes = [vp, vp, vp, vp, vp, u32, u64, u32, u32, u32, i32, i32, u32, vp, u64, vp, vp, vp, vp, vp]
    # reading TIFF files: the IFD chain, a batch inflate of strips or tiles, the predictor undo (csrc/tiff_kernels.h, zmi_api.hip)
    L.zmi_tiff_row_tile.restype = u32
    L.zmi_tiff_row_tile.argtypes = []
    L.zmi_tiff_directory_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp]
    L.zmi_tiff_read_dev.argtypes = [vp, vp, u64, vp, u32, u32, vp, u32, u64, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    # reading OpenEXR images: the attribute list, a batch inflate of the chunks, the unzip (csrc/exr_kernels.h, zmi_api.hip)
    L.zmi_exr_trip.restype = u32
    L.zmi_exr_trip.argtypes = []
    L.zmi_exr_piece.restype = u32
    L.zmi_exr_piece.argtypes = []
    L.zmi_exr_pxr24_trip.restype = u32
    L.zmi_exr_pxr24_trip.argtypes = []
    L.zmi_exr_headers_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp]
    L.zmi_exr_read_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, u32, u64, u32, u32, vp, u64, vp, vp, vp, vp, vp]
    # writing TIFF files: the forward predictor, deflate in pieces, the IFD (csrc/tiff_write_kernels.h, zmi_api.hip); w: a TiffWrite
    L.zmi_tiff_predict_tile.restype = u32
    L.zmi_tiff_predict_tile.argtypes = []
    L.zmi_tiff_bound.restype = u64
    L.zmi_tiff_bound.argtypes = [C.POINTER(TiffWrite)]
    L.zmi_tiff_write_dev.argtypes = [vp, C.POINTER(TiffWrite), vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    # writing OpenEXR images: the forward zip, deflate in pieces, chunks and offset table (csrc/exr_write_kernels.h, zmi_api.hip); w: an ExrWrite
    L.zmi_exr_zip_trip.restype = u32
    L.zmi_exr_zip_trip.argtypes = []
    L.zmi_exr_bound.restype = u64
    L.zmi_exr_bound.argtypes = [C.POINTER(ExrWrite), u32]
    L.zmi_exr_write_dev.argtypes = [vp, C.POINTER(ExrWrite), vp, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp, vp]
    # the multi-GPU stitch (csrc/exchange.hip); RCCL itself is loaded by the library on first use
    L.zmi_comm_unique_id.argtypes = [vp]
    L.zmi_comm_create.argtypes = [C.POINTER(vp), vp, i32, i32, vp]
    L.zmi_comm_destroy.argtypes = [vp]
    L.zmi_comm_abort.argtypes = [vp]
    L.zmi_exchange_sizes.argtypes = [vp, vp, u32, vp, vp]
    L.zmi_stitch_plan_dev.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.zmi_exchange_slabs.argtypes = [vp, vp, vp, vp, u64, i32, vp]
    L.zmi_exchange_slabs_round.argtypes = [vp, vp, vp, u64, u64, vp, i32, vp]
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: rc=%d (%s)" % (what, rc, lib().zmi_last_error().decode()))
