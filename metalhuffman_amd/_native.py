"""ctypes binding of libmetalhuffman_amd.so (the C-ABI in include/metalhuffman.h).

The library is loaded from this package directory only. If it is missing the
import fails loudly: there is no CPU fallback for the decode path.
"""
from __future__ import annotations

import ctypes
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MH_LIB") or os.path.join(_PKG, "libmetalhuffman_amd.so")

MH_OK = 0
MH_ERR_DIMS = -2
MH_ERR_CAPACITY = -4
MH_ERR_STREAM = -9  # a per-frame verdict of mh_check_frames / mh_check_headers: the report is not clean
MH_FLAG_NO_DELTA = 0x1
MH_FLAG_LANE_PAIRS = 0x2  # lane-pair single-frame decode: diagnostic library only (diag_lanepairs())
MH_FLAG_ANY_ORDER = 0x4  # the launch may overlap earlier work on the stream (caller guarantees independence)
MH_ENCODE_WORKSPACE_ZEROED = 0x100  # the encoder workspace was zero-filled once (mh_encode_frame_device*)
MH_ENCODE_LIMIT_LENGTHS = 0x200  # encoders only: a tree deeper than 16 gets package-merge lengths, not -3
MH_NORM_F16, MH_NORM_BF16, MH_NORM_F32 = 0, 1, 2  # mh_decode_crops_norm's element formats
MH_CROP_MIRROR = 0x1  # mh_norm_crop.flags: the crop's rows reversed along x
MH_MAX_PLANES = 4  # mh_decode_crops_norm_planes: the most planes of a sample
MH_CODES_PAD = 4
MH_TABLE2_MAX_ENTRIES = 257 * 256
MH_MAX_DIM = 65535

# every symbol include/metalhuffman.h declares
EXPORTS = (
    "mh_decode", "mh_lut_bytes", "mh_prepare_lut", "mh_lut_bits", "mh_split_blocks",
    "mh_merge_blocks", "mh_encode_signed_byte_deltas", "mh_decode_signed_byte_deltas",
    "mh_codes_bound", "mh_encode_huffman", "mh_encode_frame", "mh_canonical_codes",
    "mh_build_tables", "mh_build_single_table", "mh_error_string", "mh_device_count",
    "mh_build_tables_device", "mh_stream_create", "mh_stream_submit", "mh_stream_output",
    "mh_stream_compute_stream", "mh_stream_slot_stream", "mh_stream_wait", "mh_stream_synchronize",
    "mh_stream_destroy", "mh_stream_slot_time", "mh_stream_device",
    "mh_stream_group_create", "mh_stream_group_submit", "mh_stream_group_member", "mh_stream_group_size",
    "mh_stream_group_synchronize", "mh_stream_group_destroy",
    "mh_code_lengths", "mh_encode_workspace_bytes", "mh_encode_frame_device",
    "mh_encode_frame_device_async", "mh_encode_frames_workspace_bytes", "mh_encode_frames_device_async",
    "mh_container_header", "mh_parse_container_header", "mh_check",
    "mh_decode_huffman_bits", "mh_decode_huffman_bits_from_tables", "mh_decode_frame_cpu",
    "mh_build_stamp",
    "mh_build_luts_device", "mh_decode_frames", "mh_decode_frames_shape",
    "mh_decode_headers", "mh_decode_headers_shape", "mh_header_luts_device",
    "mh_stream_create_headers", "mh_stream_submit_header", "mh_stream_slot_status",
    "mh_code_lengths_limited",
    "mh_decode_region", "mh_decode_region_shape",
    "mh_decode_region_scaled", "mh_decode_region_scaled_shape", "mh_box_reduce",
    "mh_decode_windows", "mh_decode_windows_shape",
    "mh_decode_windows_scaled", "mh_decode_windows_scaled_shape",
    "mh_decode_crops", "mh_decode_crops_shape",
    "mh_decode_crops_norm", "mh_decode_crops_norm_shape", "mh_norm_table",
    "mh_decode_crops_norm_planes", "mh_decode_crops_norm_planes_shape",
    "mh_decode_set_crops", "mh_decode_set_crops_shape",
    "mh_decode_set_crops_norm_planes", "mh_decode_set_crops_norm_planes_shape",
    "mh_encode_frames_shared_workspace_bytes", "mh_encode_frames_shared_device_async",
    "mh_frame_histogram", "mh_encode_frame_with_header",
    "mh_encode_images_workspace_bytes", "mh_encode_images_shared_workspace_bytes",
    "mh_encode_images_device_async", "mh_encode_images_shared_device_async",
    "mh_check_frames", "mh_check_frames_shape", "mh_check_headers", "mh_check_headers_shape",
    "mh_check_frame_cpu",
    "mh_encode_set_plan_bytes", "mh_encode_set_plan", "mh_encode_set_device_async",
    "mh_decode_set_frames", "mh_decode_set_frames_shape", "mh_decode_set_plan",
    "mh_decode_marked", "mh_encode_frame_marks", "mh_mid_marks",
)


class MHError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().mh_error_string(status).decode() if _lib is not None else str(status)
        super().__init__(f"{what}: {msg} (status {status})" if what else f"{msg} (status {status})")


class mh_dims(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("block_width", ctypes.c_uint32), ("block_height", ctypes.c_uint32)]


class mh_frame(ctypes.Structure):
    _fields_ = [
        ("d_block_offsets", ctypes.c_void_p),
        ("d_codes", ctypes.c_void_p),
        ("codes_bytes", ctypes.c_uint64),
        ("d_frame_code_offsets", ctypes.c_void_p),
        ("d_table1", ctypes.c_void_p),
        ("d_table2", ctypes.c_void_p),
        ("table2_entries", ctypes.c_uint32),
        ("d_lut", ctypes.c_void_p),
        ("d_block_init", ctypes.c_void_p),
        ("dims", mh_dims),
        ("n_frames", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class mh_region(ctypes.Structure):
    _fields_ = [("bx0", ctypes.c_uint32), ("by0", ctypes.c_uint32), ("bw", ctypes.c_uint32),
                ("bh", ctypes.c_uint32)]


class mh_window(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_uint32), ("bx0", ctypes.c_uint32), ("by0", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class mh_crop(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_uint32), ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class mh_norm_crop(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_uint32), ("x0", ctypes.c_uint32), ("y0", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class mh_frame_geom(ctypes.Structure):
    _fields_ = [("first_block", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class mh_set_raster(ctypes.Structure):
    """Where mh_decode_set_frames writes frame f: row y at d_out + offset + y * pitch."""
    _fields_ = [("offset", ctypes.c_uint64), ("pitch", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class mh_set_share(ctypes.Structure):
    """How frame f's tiles are shared out: workgroups [first_group, first_group + groups) of the launch."""
    _fields_ = [("first_group", ctypes.c_uint32), ("groups", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


MH_DECODE_GROUP_WAVES = 8  # waves of a workgroup of the frame-slice kernels


class mh_image_layout(ctypes.Structure):
    _fields_ = [("image_stride", ctypes.c_uint64), ("row_pitch", ctypes.c_uint64),
                ("pixel_stride", ctypes.c_uint32), ("first_channel", ctypes.c_uint32),
                ("n_planes", ctypes.c_uint32), ("plane_major", ctypes.c_uint32)]


class mh_set_source(ctypes.Structure):
    """One frame of mh_encode_set_plan: sample (x, y) is the byte at pixels + y * row_pitch + x * pixel_stride."""
    _fields_ = [("pixels", ctypes.c_uint64), ("row_pitch", ctypes.c_uint64), ("pixel_stride", ctypes.c_uint32),
                ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("codes_cap", ctypes.c_uint64)]


class mh_set_frame(ctypes.Structure):
    """The plan's record of one frame (device format)."""
    _fields_ = [("pixels", ctypes.c_uint64), ("slot_offset", ctypes.c_uint64), ("codes_cap", ctypes.c_uint64),
                ("row_pitch", ctypes.c_uint32), ("pixel_stride", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("block_width", ctypes.c_uint32), ("n_blocks", ctypes.c_uint32),
                ("n_tiles", ctypes.c_uint32), ("first_tile", ctypes.c_uint32), ("first_block", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class mh_set_totals(ctypes.Structure):
    _fields_ = [("codes_bytes", ctypes.c_uint64), ("workspace_bytes", ctypes.c_uint64),
                ("plan_bytes", ctypes.c_uint64), ("geoms_offset", ctypes.c_uint64),
                ("split_map_offset", ctypes.c_uint64), ("pack_map_offset", ctypes.c_uint64),
                ("n_frames", ctypes.c_uint32), ("total_blocks", ctypes.c_uint32), ("total_tiles", ctypes.c_uint32),
                ("split_grid", ctypes.c_uint32), ("pack_grid", ctypes.c_uint32), ("max_width", ctypes.c_uint32),
                ("max_height", ctypes.c_uint32), ("fetch_mode", ctypes.c_uint32)]


MH_SET_TILE_BLOCKS = 256  # blocks per tile of the set encoder's maps
MH_SET_PACK_TILES = 4     # tiles of one frame per pack workgroup
MH_SET_FETCH_BYTES = 0xFF  # mh_set_totals.fetch_mode: byte loads (1..4: dword loads at that pixel stride)
MH_IMAGE_TILE_SPAN_MAX = 0x7FFFFFF0  # mh_encode_images_*: the most bytes one tile's descriptor spans


def image_tile_rows(width: int) -> int:
    """MH_IMAGE_TILE_ROWS(width): the most pixel rows one tile of 256 blocks lies in."""
    return 8 * (254 // ((width + 7) // 8) + 2)


_lib = None

_vp = ctypes.c_void_p
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u16p = ctypes.POINTER(ctypes.c_uint16)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_f32p = ctypes.POINTER(ctypes.c_float)


_diag_lp = None


def diag_lanepairs() -> ctypes.CDLL:
    """The lane-pair diagnostic library (metalhuffman_amd/diag/libmh_diag_lanepairs.so,
    built by `python -m metalhuffman_amd.build`): north_star's lane-group cursor, a
    measured negative kept for A/B and its parity tests. It exports
    one entry point, mh_diag_decode_lanepairs, with mh_decode's signature; the product
    library refuses MH_FLAG_LANE_PAIRS."""
    global _diag_lp
    if _diag_lp is None:
        from . import build as _build
        path = _build.diag_lib_path("lanepairs")
        if not os.path.exists(path):
            raise ImportError(f"{path} not found: build it with `python -m metalhuffman_amd.build`")
        L = ctypes.CDLL(path)
        L.mh_build_stamp.restype = ctypes.c_char_p
        want, have = "diag:lanepairs:" + _build.diag_stamp("lanepairs"), L.mh_build_stamp().decode()
        if have != want:
            raise ImportError(f"{path} was built from other sources: rebuild with `python -m metalhuffman_amd.build`")
        L.mh_diag_decode_lanepairs.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_size_t, ctypes.c_size_t,
                                               _vp]
        _diag_lp = L
    return _diag_lp


def has_mid_marks(L=None) -> bool:
    """The library carries the mid-block marks' entries. Always true of the product library; an
    A/B variant (MH_LIB) built from older sources has none, and frames are then encoded and
    decoded without marks."""
    return hasattr(L if L is not None else lib(), "mh_decode_marked")


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -m metalhuffman_amd.build` "
                "(the HIP decoder has no fallback)")
        L = ctypes.CDLL(LIB_PATH)
        L.mh_build_stamp.restype = ctypes.c_char_p
        if not os.environ.get("MH_LIB"):  # experiment variants (MH_LIB) carry extra -D flags
            from . import build as _build

            want, have = _build.library_stamp(), L.mh_build_stamp().decode()
            if have != want:
                raise ImportError(
                    f"{LIB_PATH} was built from other sources (stamp {have[:16]}, sources {want[:16]}): "
                    "rebuild with `python -m metalhuffman_amd.build`")
        L.mh_decode.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]
        if has_mid_marks(L):
            L.mh_decode_marked.argtypes = [ctypes.POINTER(mh_frame), _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]
            L.mh_encode_frame_marks.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                                _u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), _u32p,
                                                _u8p, _u32p]
            L.mh_mid_marks.argtypes = [_u8p, ctypes.c_uint64, _u32p, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32,
                                       _u8p, ctypes.c_uint32, _u32p]
        L.mh_check.argtypes = [ctypes.POINTER(mh_frame), _vp, _vp]
        L.mh_check_frames.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp]
        L.mh_check_headers.argtypes = [ctypes.POINTER(mh_frame), _vp, _vp, _vp, _vp, _vp, _vp]
        L.mh_check_frames_shape.argtypes = [ctypes.POINTER(mh_frame), _vp, _u32p, _u32p]
        L.mh_check_headers_shape.argtypes = [ctypes.POINTER(mh_frame), _vp, _u32p, _u32p]
        L.mh_check_frame_cpu.argtypes = [_u32p, ctypes.c_uint32, _u8p, ctypes.c_uint64, _u8p, _u32p]
        L.mh_lut_bytes.restype = ctypes.c_size_t
        L.mh_lut_bits.restype = ctypes.c_int
        L.mh_prepare_lut.argtypes = [_vp, _vp, ctypes.c_uint32, _vp, _vp]
        L.mh_build_tables_device.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.mh_build_luts_device.argtypes = [_vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp]
        L.mh_decode_frames.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_size_t,
                                       ctypes.c_size_t, _vp]
        L.mh_decode_frames_shape.argtypes = [ctypes.POINTER(mh_frame), _vp, _u32p, _u32p]
        L.mh_decode_headers.argtypes = [ctypes.POINTER(mh_frame), _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                        ctypes.c_size_t, _vp]
        L.mh_decode_headers_shape.argtypes = [ctypes.POINTER(mh_frame), _vp, _u32p, _u32p]
        L.mh_decode_region.argtypes = [ctypes.POINTER(mh_frame), ctypes.POINTER(mh_region), _vp, ctypes.c_uint64, _vp,
                                       _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]
        L.mh_decode_region_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.POINTER(mh_region), _vp, _u32p, _u32p]
        L.mh_decode_region_scaled.argtypes = [ctypes.POINTER(mh_frame), ctypes.POINTER(mh_region), ctypes.c_uint32,
                                              _vp, ctypes.c_uint64, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]
        L.mh_decode_region_scaled_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.POINTER(mh_region),
                                                    ctypes.c_uint32, _vp, _u32p, _u32p]
        L.mh_decode_windows.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_size_t,
                                        ctypes.c_size_t, _vp]
        L.mh_decode_windows_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint32, _vp, _u32p, _u32p]
        L.mh_decode_windows_scaled.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                               ctypes.c_size_t, ctypes.c_size_t, _vp]
        L.mh_decode_windows_scaled_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32, ctypes.c_uint32,
                                                     ctypes.c_uint32, ctypes.c_uint32, _vp, _u32p, _u32p]
        L.mh_decode_crops.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_size_t,
                                      ctypes.c_size_t, _vp]
        L.mh_decode_crops_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, _vp, _u32p, _u32p]
        L.mh_decode_crops_norm.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_float, _vp,
                                           ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _vp]
        L.mh_decode_crops_norm_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_uint32, _vp, _u32p, _u32p]
        L.mh_norm_table.argtypes = [ctypes.c_uint32, ctypes.c_float, ctypes.c_float, _vp, ctypes.c_size_t]
        L.mh_decode_crops_norm_planes.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, ctypes.c_uint32,
                                                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                  _f32p, _f32p, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_size_t,
                                                  ctypes.c_size_t, ctypes.c_size_t, _vp]
        L.mh_decode_crops_norm_planes_shape.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32, ctypes.c_uint32,
                                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _u32p,
                                                        _u32p]
        # the set entries: their parents' lists with (d_geoms, total_blocks) behind the frame; the
        # *_shape twins are the parents'
        for name in ("mh_decode_crops", "mh_decode_crops_norm_planes"):
            args = getattr(L, name).argtypes
            set_name = name.replace("mh_decode_", "mh_decode_set_")
            getattr(L, set_name).argtypes = [args[0], _vp, ctypes.c_uint32] + list(args[1:])
            getattr(L, set_name + "_shape").argtypes = getattr(L, name + "_shape").argtypes
        L.mh_decode_set_frames.argtypes = [ctypes.POINTER(mh_frame), _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                           ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint64, _vp]
        L.mh_decode_set_frames_shape.argtypes = [ctypes.POINTER(mh_frame), _vp, _u32p, _u32p]
        L.mh_decode_set_plan.argtypes = [ctypes.c_uint32, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                         ctypes.c_uint32, _u32p, _u64p]
        L.mh_box_reduce.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_uint32, _vp,
                                    ctypes.c_size_t]
        L.mh_header_luts_device.argtypes = [_vp, ctypes.c_uint32, _vp, ctypes.c_uint64, _vp, _vp]
        L.mh_stream_create_headers.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint64, ctypes.c_uint32,
                                               ctypes.POINTER(_vp), ctypes.POINTER(_vp)]
        L.mh_stream_submit_header.argtypes = [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _u32p]
        L.mh_stream_slot_status.argtypes = [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
        L.mh_stream_create.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint64, ctypes.c_uint32,
                                       ctypes.POINTER(_vp), ctypes.POINTER(_vp)]
        L.mh_stream_submit.argtypes = [_vp, _vp, ctypes.c_uint64, _vp, _vp, _u32p]
        L.mh_stream_output.argtypes = [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_size_t)]
        L.mh_stream_output.restype = _vp
        L.mh_stream_compute_stream.argtypes = [_vp]
        L.mh_stream_compute_stream.restype = _vp
        L.mh_stream_slot_stream.argtypes = [_vp, ctypes.c_uint32]
        L.mh_stream_slot_stream.restype = _vp
        L.mh_stream_wait.argtypes = [_vp, ctypes.c_uint32]
        L.mh_stream_synchronize.argtypes = [_vp]
        L.mh_stream_destroy.argtypes = [_vp]
        L.mh_stream_slot_time.argtypes = [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
        L.mh_stream_device.argtypes = [_vp]
        L.mh_stream_group_create.argtypes = [ctypes.POINTER(mh_frame), ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_int), ctypes.c_uint64, ctypes.c_uint32,
                                             ctypes.POINTER(_vp)]
        L.mh_stream_group_submit.argtypes = [_vp, _vp, ctypes.c_uint64, _vp, _vp, _u32p, _u32p]
        L.mh_stream_group_member.argtypes = [_vp, ctypes.c_uint32]
        L.mh_stream_group_member.restype = _vp
        L.mh_stream_group_size.argtypes = [_vp]
        L.mh_stream_group_size.restype = ctypes.c_uint32
        L.mh_stream_group_synchronize.argtypes = [_vp]
        L.mh_stream_group_destroy.argtypes = [_vp]
        L.mh_code_lengths.argtypes = [_u64p, _u8p]
        L.mh_code_lengths_limited.argtypes = [_u64p, ctypes.c_uint32, _u8p]
        L.mh_container_header.argtypes = [ctypes.c_uint64, _u8p]
        L.mh_parse_container_header.argtypes = [_u8p, _u64p]
        L.mh_encode_workspace_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        L.mh_encode_workspace_bytes.restype = ctypes.c_size_t
        L.mh_encode_frame_device.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                             _vp, ctypes.c_uint64, _u64p, _vp, _vp, _vp, ctypes.c_size_t,
                                             _vp]
        L.mh_encode_frame_device_async.argtypes = [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                   _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp,
                                                   ctypes.c_size_t, _vp]
        L.mh_encode_frames_workspace_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.mh_encode_frames_workspace_bytes.restype = ctypes.c_size_t
        L.mh_encode_frames_device_async.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                                    _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.mh_encode_frames_shared_workspace_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.mh_encode_frames_shared_workspace_bytes.restype = ctypes.c_size_t
        L.mh_encode_frames_shared_device_async.argtypes = [_vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                           ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp,
                                                           ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                           ctypes.c_size_t, _vp]
        for name in ("mh_encode_images_workspace_bytes", "mh_encode_images_shared_workspace_bytes"):
            getattr(L, name).argtypes = [ctypes.c_uint32] * 4
            getattr(L, name).restype = ctypes.c_size_t
        L.mh_encode_images_device_async.argtypes = (
            [_vp, ctypes.POINTER(mh_image_layout)] + L.mh_encode_frames_device_async.argtypes[2:])
        L.mh_encode_images_shared_device_async.argtypes = (
            [_vp, ctypes.POINTER(mh_image_layout)] + L.mh_encode_frames_shared_device_async.argtypes[2:])
        L.mh_encode_set_plan_bytes.argtypes = [ctypes.c_uint32, ctypes.POINTER(mh_set_source)]
        L.mh_encode_set_plan_bytes.restype = ctypes.c_size_t
        L.mh_encode_set_plan.argtypes = [ctypes.c_uint32, ctypes.POINTER(mh_set_source), ctypes.c_uint32, _vp,
                                         ctypes.c_size_t, ctypes.POINTER(mh_set_totals)]
        L.mh_encode_set_device_async.argtypes = [_vp, ctypes.POINTER(mh_set_totals), ctypes.c_uint32, _vp, _vp,
                                                 ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.mh_frame_histogram.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                         _u64p]
        L.mh_encode_frame_with_header.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                                  _u8p, ctypes.c_uint64, _u64p, _u32p, _u8p]
        L.mh_split_blocks.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint8, _u8p, ctypes.c_size_t]
        L.mh_merge_blocks.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                      ctypes.c_size_t]
        L.mh_encode_signed_byte_deltas.argtypes = [_u8p, _u8p, ctypes.c_size_t]
        L.mh_decode_signed_byte_deltas.argtypes = [_u8p, _u8p, ctypes.c_size_t]
        L.mh_codes_bound.argtypes = [ctypes.c_uint64]
        L.mh_codes_bound.restype = ctypes.c_uint64
        L.mh_encode_huffman.argtypes = [_u8p, ctypes.c_uint64, ctypes.c_uint32, _u8p, _u8p,
                                        ctypes.c_uint64, _u64p, _u32p]
        L.mh_encode_frame.argtypes = [_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                      _u8p, ctypes.c_uint64, _u64p, _u32p, _u8p]
        L.mh_canonical_codes.argtypes = [_u8p, _u16p]
        L.mh_build_tables.argtypes = [_u8p, _u8p, _u8p, ctypes.c_uint32, _u32p]
        L.mh_build_single_table.argtypes = [_u8p, _u8p]
        L.mh_decode_huffman_bits.argtypes = [_u8p, ctypes.c_uint64, _u8p, ctypes.c_uint64, _u8p, _u32p]
        L.mh_decode_huffman_bits_from_tables.argtypes = [_u8p, _u8p, ctypes.c_uint32, ctypes.c_uint32,
                                                         ctypes.c_uint32, ctypes.c_uint64, _u8p,
                                                         ctypes.c_uint64, _u8p, _u32p]
        L.mh_decode_frame_cpu.argtypes = [_u32p, _u8p, ctypes.c_uint64, _u8p, _u8p, ctypes.c_uint32, _u8p,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _u8p,
                                          ctypes.c_size_t, ctypes.c_uint32]
        L.mh_error_string.argtypes = [ctypes.c_int]
        L.mh_error_string.restype = ctypes.c_char_p
        L.mh_device_count.restype = ctypes.c_int
        _lib = L
    return _lib


def check(status: int, what: str = "") -> None:
    if status != MH_OK:
        raise MHError(status, what)
