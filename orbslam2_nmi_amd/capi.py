"""ctypes view of the C ABI in include/nmi_hip.h (libnmi_hip.so).

There is no CPU fallback here: if the HIP library is missing or cannot be loaded this module raises,
and every entry point requires device (torch CUDA/HIP) tensors.  torch is used only to own device
memory and streams; the compute is the hand-written HIP in csrc/.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MODE_ENMI = 0  # Thirdparty/CUDA_Functions/kernel.cuh:22
MODE_SUC = 1   # Thirdparty/CUDA_Functions/kernel.cuh:23

NMI_OK = 0
ERR_INVALID_ARGUMENT = -1
ERR_UNSUPPORTED = -2
ERR_NO_DEVICE = -3
ERR_NOT_READY = -4

# Camera frame formats (include/nmi_hip.h, nmi_gray_frame): bytes per pixel 1, 3, 3, 4, 4; Camera.RGB 0 -> BGR(A), 1 -> RGB(A).
FRAME_GRAY = 0
FRAME_BGR = 1
FRAME_RGB = 2
FRAME_BGRA = 3
FRAME_RGBA = 4
# Raw sensor formats: packed YUV 4:2:2 (the luma byte is the grey value) and 8-bit Bayer mosaics (named by the 2x2 tile at (0, 0)).
FRAME_YUYV = 16
FRAME_UYVY = 17
FRAME_BAYER_RGGB = 32
FRAME_BAYER_GRBG = 33
FRAME_BAYER_GBRG = 34
FRAME_BAYER_BGGR = 35
# Deep grey frames: 2 bytes per pixel, little-endian unsigned, made 8-bit by a tone map (ToneMap, TONE_*).
FRAME_GRAY16 = 48
# Deep raw formats, each unpacked on the device to the GRAY16 container: big-endian words, PFNC Mono10p / Mono12p (lsb-packed), CSI-2
# RAW10 / RAW12 (V4L2 Y10P / Y12P) and 16-bit Bayer mosaics (2 bytes per site, little-endian).
FRAME_GRAY16_BE = 50
FRAME_MONO10P = 52
FRAME_MONO12P = 53
FRAME_RAW10 = 54
FRAME_RAW12 = 55
FRAME_BAYER16_RGGB = 56
FRAME_BAYER16_GRBG = 57
FRAME_BAYER16_GBRG = 58
FRAME_BAYER16_BGGR = 59
FRAME_UNPACKED = (FRAME_GRAY16_BE, FRAME_MONO10P, FRAME_MONO12P, FRAME_RAW10, FRAME_RAW12, FRAME_BAYER16_RGGB, FRAME_BAYER16_GRBG,
                  FRAME_BAYER16_GBRG, FRAME_BAYER16_BGGR)
# (the byte-packed formats have no whole number of bytes per pixel: frame_row_bytes)
FRAME_BYTES_PER_PIXEL = {FRAME_GRAY: 1, FRAME_BGR: 3, FRAME_RGB: 3, FRAME_BGRA: 4, FRAME_RGBA: 4, FRAME_YUYV: 2, FRAME_UYVY: 2,
                         FRAME_BAYER_RGGB: 1, FRAME_BAYER_GRBG: 1, FRAME_BAYER_GBRG: 1, FRAME_BAYER_BGGR: 1, FRAME_GRAY16: 2,
                         FRAME_GRAY16_BE: 2, FRAME_BAYER16_RGGB: 2, FRAME_BAYER16_GRBG: 2, FRAME_BAYER16_GBRG: 2, FRAME_BAYER16_BGGR: 2}


def frame_row_bytes(fmt, width):
    """nmi_frame_row_bytes: the dense bytes of a row of `width` pixels in format fmt (FRAME_*); 0 for an unknown format or a width
    that is not whole groups (4 pixels in 5 bytes for the 10-bit packed formats, 2 in 3 for the 12-bit ones).  Host only."""
    lib = load_library()
    if not hasattr(lib, "nmi_frame_row_bytes"):  # (a library of an earlier commit, loaded for A/B timing: whole bytes per pixel only)
        return max(int(width), 0) * FRAME_BYTES_PER_PIXEL.get(int(fmt), 0)
    return int(lib.nmi_frame_row_bytes(int(fmt), int(width)))


def _frame_bytes(fmt, pitch, width, height):
    """Bytes from a frame's first to the end of its last row's pixels, or None where the library will refuse the arguments."""
    row = frame_row_bytes(fmt, width)
    return (height - 1) * (int(pitch) or row) + row if row > 0 and int(pitch) >= 0 else None
TONE_SHIFT = 0
TONE_WINDOW = 1
TONE_PERCENTILE = 2
TONE_EQUALIZE = 3
TONE_TABLE = 4
TONE_CLAHE = 6       # (5 stays an unknown mode)
TONE_LEVELS = 65536  # entries of a tone table
TONE_MAX_TILES = 8   # CLAHE: tiles per axis

# Every symbol include/nmi_hip.h declares; tests check that the library exports all of them.
EXPORTED_SYMBOLS = (
    "nmi_params_default", "nmi_create", "nmi_destroy", "nmi_set_stream", "nmi_synchronize", "nmi_eval_pair", "nmi_eval_pairs", "nmi_eval_pair_debug",
    "nmi_search_grid", "nmi_search_grid_shard", "nmi_search_grid_block", "nmi_warp_homographies", "nmi_warp_stack", "nmi_render_mvp", "nmi_render_points", "nmi_level_create", "nmi_level_create_mesh", "nmi_level_run", "nmi_level_copy_outputs", "nmi_level_destroy", "nmi_texture_create",
    "nmi_texture_destroy", "nmi_render_mesh", "nmi_stream_create", "nmi_stream_destroy",
    "nmi_stream_submit", "nmi_stream_wait", "nmi_stream_keep_ratings", "nmi_stream_copy_ratings", "nmi_key_pack", "nmi_key_unpack", "nmi_search_grid_rccl", "nmi_search_grid_block_rccl",
    "nmi_rccl_unique_id", "nmi_rccl_comm_init", "nmi_rccl_comm_destroy", "nmi_set_profiling", "nmi_last_kernel_ms",
    "nmi_set_option", "nmi_copy_term_table", "nmi_abi_version", "nmi_error_string", "nmi_last_error_detail", "nmi_get_info", "nmi_last_content", "nmi_sort_points", "nmi_sort_triangles",
    "nmi_split_status", "nmi_pix_status", "nmi_pix_heal_counts", "nmi_level_create_block", "nmi_level_create_mesh_block", "nmi_level_run_rccl", "nmi_stream_submit_block",
    "nmi_warp_stack_masked", "nmi_search_grid_masked", "nmi_last_mask_counts", "nmi_level_set_masks", "nmi_level_copy_masks",
    "nmi_render_points_masked", "nmi_render_mesh_masked", "nmi_search_grid_covered", "nmi_last_cover_counts",
    "nmi_level_set_coverage", "nmi_level_copy_coverage",
    "nmi_pack_mask_bits", "nmi_stream_submit_masked", "nmi_stream_submit_masked_block", "nmi_stream_submit_covered",
    "nmi_stream_submit_covered_block", "nmi_stream_copy_counts",
    "nmi_undistort_frame", "nmi_level_set_distortion", "nmi_stream_set_distortion",
    "nmi_gray_frame", "nmi_level_set_frame_format", "nmi_stream_set_frame_format",
    "nmi_reduce_frame", "nmi_level_set_frame_reduction", "nmi_stream_set_frame_reduction",
    "nmi_render_mesh_colored", "nmi_render_mesh_colored_masked", "nmi_sort_triangles_colored", "nmi_level_create_mesh_colored",
    "nmi_level_create_mesh_colored_block",
    "nmi_undistort_frame_fisheye", "nmi_level_set_distortion_fisheye", "nmi_stream_set_distortion_fisheye",
    "nmi_tone_map_default", "nmi_set_tone_map", "nmi_level_set_tone_map", "nmi_stream_set_tone_map", "nmi_tone_lut",
    "nmi_tone_tile_luts",
    "nmi_set_valid_range", "nmi_deep_frame",
    "nmi_frame_row_bytes", "nmi_unpack_frame",
    "nmi_level_set_valid_range", "nmi_stream_set_valid_range",
    "nmi_render_points_depth", "nmi_render_mesh_depth", "nmi_depth_shade_apply",
    "nmi_level_create_depth", "nmi_level_create_depth_block", "nmi_level_set_depth_shade",
    "nmi_rank_peaks", "nmi_level_set_peaks", "nmi_level_copy_peaks",
    "nmi_refine_peaks", "nmi_level_set_refine", "nmi_level_copy_refined",
)
PEAKS_MAX_K = 64   # nmi_rank_peaks: keys per call
# nmi_refined_peak (include/nmi_refined_peak.h), 152 bytes, and its flags
REFINED_PEAK = np.dtype([("key", np.uint64), ("offset", np.float32, 6), ("score", np.float32), ("flags", np.uint32),
                         ("gradient", np.float32, 6), ("hessian", np.float32, 21), ("reserved", np.uint32)])
assert REFINED_PEAK.itemsize == 152
REFINE_EMPTY, REFINE_NONFINITE, REFINE_COUPLED, REFINE_CROSS_HOLE = 1, 2, 4, 8


def refine_border(a):
    return 0x100 << a


def refine_hole(a):
    return 0x10000 << a


def refine_flat(a):
    return 0x1000000 << a


MAP_POINTS = 0   # nmi_level_create_depth's map_kind
MAP_MESH = 1


class NmiParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("bins", C.c_int32), ("mode", C.c_int32),
        ("use_bg", C.c_int32), ("render_bottom_up", C.c_int32), ("device", C.c_int32),
        ("max_candidates", C.c_int32), ("stream", C.c_void_p), ("reserved", C.c_int32 * 8),
    ]


class ToneMap(C.Structure):
    """nmi_tone_map (include/nmi_hip.h, "Deep frames"): how a FRAME_GRAY16 pixel becomes 8-bit.  The constructors below fill the
    fields of their mode; `table` keeps the device tensor of a TABLE alive as long as the value."""
    _fields_ = [("mode", C.c_int32), ("bits", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("p_lo", C.c_int32),
                ("p_hi", C.c_int32), ("plateau", C.c_int32), ("reserved", C.c_int32 * 5), ("d_lut", C.c_void_p)]
    table = None

    # CLAHE's tile counts are the first two of the header's five former reserved words (tiles_x, tiles_y, reserved[3]).
    @property
    def tiles_x(self):
        return int(self.reserved[0])

    @tiles_x.setter
    def tiles_x(self, n):
        self.reserved[0] = int(n)

    @property
    def tiles_y(self):
        return int(self.reserved[1])

    @tiles_y.setter
    def tiles_y(self, n):
        self.reserved[1] = int(n)

    @classmethod
    def clahe(cls, tiles_x=8, tiles_y=8, plateau=0, bits=16):
        """Contrast-limited equalisation per tile (TONE_CLAHE): tiles_x x tiles_y tiles, 1 .. TONE_MAX_TILES each and no more
        than the context's width and height; plateau: the per-level count limit within a tile, 0 = none."""
        tm = cls(mode=TONE_CLAHE, bits=bits, plateau=plateau)
        tm.tiles_x, tm.tiles_y = tiles_x, tiles_y
        return tm

    @classmethod
    def shift(cls, bits=16):
        return cls(mode=TONE_SHIFT, bits=bits)

    @classmethod
    def window(cls, lo, hi, bits=16):
        return cls(mode=TONE_WINDOW, bits=bits, lo=lo, hi=hi)

    @classmethod
    def percentile(cls, p_lo=0, p_hi=0, bits=16):
        return cls(mode=TONE_PERCENTILE, bits=bits, p_lo=p_lo, p_hi=p_hi)

    @classmethod
    def equalize(cls, plateau=0, bits=16):
        return cls(mode=TONE_EQUALIZE, bits=bits, plateau=plateau)

    @classmethod
    def from_table(cls, lut, bits=16):
        """lut: device uint8 tensor of TONE_LEVELS entries (tone_lut makes one); it must stay unchanged while the setting holds."""
        if not (lut.is_cuda and str(lut.dtype) == "torch.uint8" and lut.is_contiguous() and lut.numel() == TONE_LEVELS):
            raise TypeError(f"lut must be a contiguous device uint8 tensor of {TONE_LEVELS} entries")
        tm = cls(mode=TONE_TABLE, bits=bits, d_lut=lut.data_ptr())
        tm.table = lut
        return tm


def _tone_ref(tm):
    """The argument of a set_tone_map call: None -> NULL (the default setting)."""
    if tm is None:
        return None
    if not isinstance(tm, ToneMap):
        raise TypeError("tone map must be a ToneMap or None")
    return C.byref(tm)


class NmiDepthShade(C.Structure):
    """nmi_depth_shade (include/nmi_hip.h, "Depth maps"): how a depth render turns the winner's window depth into a raw 16-bit
    depth (near_plane / far_plane of the projection, scale raw units per world unit) and that into grey (the window lo < hi,
    NMI_TONE_WINDOW's rule)."""
    _fields_ = [("near_plane", C.c_float), ("far_plane", C.c_float), ("scale", C.c_float), ("lo", C.c_int32), ("hi", C.c_int32),
                ("reserved", C.c_int32 * 3)]


def _shade_ref(shade, allow_none=False):
    if shade is None and allow_none:
        return None
    if not isinstance(shade, NmiDepthShade):
        raise TypeError("shade must be an NmiDepthShade")
    return C.byref(shade)


class RenderParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("near_plane", C.c_float),
                ("far_plane", C.c_float), ("point_size", C.c_float)]


class NmiError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        super().__init__(f"{what} failed: {code} ({error_string(code)}) {detail}".strip())


_lib = None


def library_path():
    return _build.LIB


def load_library(build_if_missing=False):
    """Loads libnmi_hip.so.  Raises if it is not there (the product has no other compute path)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if build_if_missing:
        _build.build()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -m orbslam2_nmi_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback for the NMI path.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, i32, i64p, f32p, u64p = C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    lib.nmi_params_default.argtypes = [C.POINTER(NmiParams), i32, i32]
    lib.nmi_create.argtypes = [C.POINTER(NmiParams), C.POINTER(vp)]
    lib.nmi_destroy.argtypes = [vp]
    lib.nmi_set_stream.argtypes = [vp, vp]
    lib.nmi_synchronize.argtypes = [vp]
    lib.nmi_eval_pair.argtypes = [vp, vp, vp, f32p]
    lib.nmi_eval_pairs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32, f32p]
    lib.nmi_eval_pair_debug.argtypes = [vp, vp, vp, f32p, vp, vp, vp, vp]
    lib.nmi_search_grid.argtypes = [vp, vp, i32, vp, i32, vp, i64p, f32p]
    lib.nmi_search_grid_shard.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp, u64p]
    lib.nmi_search_grid_block.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, u64p]
    lib.nmi_warp_homographies.argtypes = [C.POINTER(C.c_double), C.POINTER(i32), f32p, C.POINTER(C.c_double)]
    lib.nmi_warp_stack.argtypes = [vp, vp, C.POINTER(C.c_double), i32, vp]
    lib.nmi_warp_stack_masked.argtypes = [vp, vp, vp, C.POINTER(C.c_double), i32, vp, vp]
    lib.nmi_search_grid_masked.argtypes = [vp, vp, i32, vp, vp, i32, vp, i64p, f32p]
    lib.nmi_last_mask_counts.argtypes = [vp, C.POINTER(i32), i32]
    lib.nmi_render_points_masked.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_float), i32, C.c_float, vp, vp]
    lib.nmi_render_mesh_masked.argtypes = [vp, vp, vp, C.c_int64, vp, C.POINTER(C.c_float), i32, vp, vp]
    lib.nmi_search_grid_covered.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, i64p, f32p]
    lib.nmi_last_cover_counts.argtypes = [vp, C.POINTER(i32), i32]
    lib.nmi_render_mvp.argtypes = [C.POINTER(RenderParams), f32p, f32p, f32p, f32p, f32p]
    lib.nmi_render_points.argtypes = [vp, vp, vp, C.c_int64, f32p, i32, C.c_float, vp]
    lib.nmi_texture_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    lib.nmi_texture_destroy.argtypes = [vp]
    lib.nmi_render_mesh.argtypes = [vp, vp, vp, C.c_int64, vp, f32p, i32, vp]
    lib.nmi_level_create.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, C.c_float, C.POINTER(vp)]
    lib.nmi_level_create_mesh.argtypes = [vp, vp, vp, C.c_int64, vp, vp, i32, i32, C.POINTER(vp)]
    lib.nmi_level_run.argtypes = [vp, f32p, C.POINTER(C.c_double), i64p, f32p]
    lib.nmi_level_create_block.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, i32, i32, C.c_float, C.POINTER(vp)]
    lib.nmi_level_create_mesh_block.argtypes = [vp, vp, vp, C.c_int64, vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.nmi_render_mesh_colored.argtypes = [vp, vp, vp, C.c_int64, f32p, i32, vp]
    lib.nmi_render_mesh_colored_masked.argtypes = [vp, vp, vp, C.c_int64, f32p, i32, vp, vp]
    lib.nmi_sort_triangles_colored.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.nmi_level_create_mesh_colored.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, C.POINTER(vp)]
    lib.nmi_level_create_mesh_colored_block.argtypes = [vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.nmi_level_run_rccl.argtypes = [vp, f32p, C.POINTER(C.c_double), vp, i64p, f32p]
    lib.nmi_stream_submit_block.argtypes = [vp, vp, i32, i32, i32, vp, C.POINTER(C.c_double), i32, i32, i32, vp, i64p]
    lib.nmi_level_copy_outputs.argtypes = [vp, vp, vp, vp]
    lib.nmi_level_set_masks.argtypes = [vp, i32, vp]
    lib.nmi_level_copy_masks.argtypes = [vp, vp, C.POINTER(i32)]
    lib.nmi_level_set_coverage.argtypes = [vp, i32, vp]
    lib.nmi_level_copy_coverage.argtypes = [vp, vp, vp, C.POINTER(i32)]
    lib.nmi_level_destroy.argtypes = [vp]
    lib.nmi_stream_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    lib.nmi_stream_destroy.argtypes = [vp]
    lib.nmi_stream_submit.argtypes = [vp, vp, i32, vp, C.POINTER(C.c_double), i32, i64p]
    lib.nmi_stream_wait.argtypes = [vp, C.c_int64, i64p, f32p]
    lib.nmi_stream_keep_ratings.argtypes = [vp, i32]
    lib.nmi_stream_copy_ratings.argtypes = [vp, C.c_int64, f32p, C.c_int64]
    lib.nmi_pack_mask_bits.argtypes = [vp, vp, i32, vp]
    lib.nmi_stream_submit_masked.argtypes = [vp, vp, i32, vp, vp, C.POINTER(C.c_double), i32, i64p]
    lib.nmi_stream_submit_masked_block.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.POINTER(C.c_double), i32, i32, i32, vp, i64p]
    lib.nmi_stream_submit_covered.argtypes = [vp, vp, vp, i32, vp, vp, C.POINTER(C.c_double), i32, i64p]
    lib.nmi_stream_submit_covered_block.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, C.POINTER(C.c_double), i32, i32, i32, vp, i64p]
    lib.nmi_stream_copy_counts.argtypes = [vp, C.c_int64, C.POINTER(i32), C.c_int64]
    lib.nmi_undistort_frame.argtypes = [vp, C.POINTER(C.c_double), f32p, vp, vp, vp, vp]
    lib.nmi_level_set_distortion.argtypes = [vp, C.POINTER(C.c_double), f32p]
    lib.nmi_stream_set_distortion.argtypes = [vp, C.POINTER(C.c_double), f32p]
    lib.nmi_undistort_frame_fisheye.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), f32p, vp, vp, vp, vp]
    lib.nmi_level_set_distortion_fisheye.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), f32p]
    lib.nmi_stream_set_distortion_fisheye.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), f32p]
    lib.nmi_gray_frame.argtypes = [vp, vp, i32, C.c_int64, vp]
    lib.nmi_level_set_frame_format.argtypes = [vp, i32, C.c_int64]
    lib.nmi_stream_set_frame_format.argtypes = [vp, i32, C.c_int64]
    lib.nmi_reduce_frame.argtypes = [vp, vp, i32, C.c_int64, i32, vp, vp, vp]
    lib.nmi_level_set_frame_reduction.argtypes = [vp, i32, i32, C.c_int64]
    lib.nmi_stream_set_frame_reduction.argtypes = [vp, i32, i32, C.c_int64]
    if hasattr(lib, "nmi_tone_map_default"):  # (absent from a library of an earlier commit loaded through NMI_HIP_LIBRARY for A/B timing)
        lib.nmi_tone_map_default.argtypes = [C.POINTER(ToneMap)]
        lib.nmi_set_tone_map.argtypes = [vp, C.POINTER(ToneMap)]
        lib.nmi_level_set_tone_map.argtypes = [vp, C.POINTER(ToneMap)]
        lib.nmi_stream_set_tone_map.argtypes = [vp, C.POINTER(ToneMap)]
        lib.nmi_tone_lut.argtypes = [vp, vp, C.c_int64, i32, vp, C.POINTER(i32)]
    if hasattr(lib, "nmi_tone_tile_luts"):
        lib.nmi_tone_tile_luts.argtypes = [vp, vp, C.c_int64, i32, vp, C.POINTER(i32)]
    if hasattr(lib, "nmi_set_valid_range"):
        lib.nmi_set_valid_range.argtypes = [vp, i32, i32]
        lib.nmi_deep_frame.argtypes = [vp, vp, C.c_int64, i32, vp, vp, vp]
    if hasattr(lib, "nmi_frame_row_bytes"):
        lib.nmi_frame_row_bytes.argtypes = [i32, i32]
        lib.nmi_frame_row_bytes.restype = C.c_int64
        lib.nmi_unpack_frame.argtypes = [vp, vp, i32, C.c_int64, i32, vp]
    if hasattr(lib, "nmi_level_set_valid_range"):
        lib.nmi_level_set_valid_range.argtypes = [vp, i32, i32]
        lib.nmi_stream_set_valid_range.argtypes = [vp, i32, i32]
    if hasattr(lib, "nmi_render_points_depth"):
        sp = C.POINTER(NmiDepthShade)
        lib.nmi_render_points_depth.argtypes = [vp, vp, vp, C.c_int64, f32p, i32, C.c_float, sp, vp, vp, vp]
        lib.nmi_render_mesh_depth.argtypes = [vp, vp, C.c_int64, f32p, i32, sp, vp, vp, vp]
        lib.nmi_depth_shade_apply.argtypes = [vp, sp, vp, C.c_int64, vp, vp]
        lib.nmi_level_create_depth.argtypes = [vp, i32, vp, C.c_int64, vp, i32, i32, C.c_float, sp, C.POINTER(vp)]
        lib.nmi_level_create_depth_block.argtypes = [vp, i32, vp, C.c_int64, vp, i32, i32, i32, i32, i32, i32, C.c_float, sp, C.POINTER(vp)]
        lib.nmi_level_set_depth_shade.argtypes = [vp, sp]
    if hasattr(lib, "nmi_rank_peaks"):
        lib.nmi_rank_peaks.argtypes = [vp, vp, C.POINTER(i32), i32, C.POINTER(i32), vp, u64p, C.POINTER(i32)]
        lib.nmi_level_set_peaks.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
        lib.nmi_level_copy_peaks.argtypes = [vp, u64p, C.POINTER(i32)]
    if hasattr(lib, "nmi_refine_peaks"):
        lib.nmi_refine_peaks.argtypes = [vp, vp, C.POINTER(i32), vp, u64p, i32, vp, vp]
        lib.nmi_level_set_refine.argtypes = [vp, i32]
        lib.nmi_level_copy_refined.argtypes = [vp, vp, C.POINTER(i32)]
    lib.nmi_key_pack.argtypes = [C.c_float, C.c_int64]
    lib.nmi_key_pack.restype = C.c_uint64
    lib.nmi_key_unpack.argtypes = [C.c_uint64, i64p, f32p]
    lib.nmi_search_grid_rccl.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp, i64p, f32p]
    lib.nmi_search_grid_block_rccl.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, i64p, f32p]
    lib.nmi_rccl_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    lib.nmi_rccl_comm_init.argtypes = [vp, C.POINTER(C.c_uint8), i32, i32, C.POINTER(vp)]
    lib.nmi_rccl_comm_destroy.argtypes = [vp]
    lib.nmi_set_option.argtypes = [vp, i32, C.c_int64]
    lib.nmi_set_profiling.argtypes = [vp, i32]
    lib.nmi_last_kernel_ms.argtypes = [vp, f32p]
    lib.nmi_copy_term_table.argtypes = [vp, f32p, C.c_int64]
    lib.nmi_error_string.argtypes = [C.c_int]
    lib.nmi_error_string.restype = C.c_char_p
    lib.nmi_last_error_detail.argtypes = [vp]
    lib.nmi_last_error_detail.restype = C.c_char_p
    lib.nmi_get_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.nmi_last_content.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.nmi_split_status.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.nmi_pix_status.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.nmi_pix_heal_counts.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.nmi_sort_points.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    lib.nmi_sort_triangles.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
    _lib = lib
    return lib


def error_string(code):
    return load_library().nmi_error_string(int(code)).decode()


def key_pack(score, index):
    return int(load_library().nmi_key_pack(float(score), int(index)))


def key_unpack(key):
    idx, sc = C.c_int64(0), C.c_float(0)
    load_library().nmi_key_unpack(C.c_uint64(int(key) & 0xFFFFFFFFFFFFFFFF), C.byref(idx), C.byref(sc))
    return int(idx.value), np.float32(sc.value)


def warp_homographies(K, num_warp_xyz, step_rad_xyz):
    """K*Rz*Ry*Rx*K^-1 per warp cell (image.cpp:76-107) -> float64 [Wn, 3, 3], w = (wz*ny + wy)*nx + wx."""
    K = np.ascontiguousarray(K, np.float64).reshape(9)
    num = (C.c_int32 * 3)(*[int(n) for n in num_warp_xyz])
    step = (C.c_float * 3)(*[float(s) for s in step_rad_xyz])
    wn = int(np.prod([int(n) for n in num_warp_xyz]))
    out = np.zeros((wn, 3, 3), np.float64)
    rc = load_library().nmi_warp_homographies(K.ctypes.data_as(C.POINTER(C.c_double)), num, step,
                                              out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != NMI_OK:
        raise NmiError(rc, "nmi_warp_homographies")
    return out


def render_mvp(rp, cam_pos, cam_look_at, cam_up, translation):
    """Projection * glm::lookAt(pos + t, look_at + t, up) as rendering.hpp:196-202,547-553 -> float32 [16], column-major."""
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    out = (C.c_float * 16)()
    rc = load_library().nmi_render_mvp(C.byref(rp), f3(cam_pos), f3(cam_look_at), f3(cam_up), f3(translation), out)
    if rc != NMI_OK:
        raise NmiError(rc, "nmi_render_mvp")
    return np.array(out, np.float32)


def _lens(K, dist):
    """(K [3,3] or [9] float64, dist [5] float32 or None) -> numpy copies and the pointers the C ABI takes (dist None -> NULL)."""
    if K is None and dist is None:
        return None, None, None, None
    k = np.ascontiguousarray(K, np.float64).reshape(-1)
    if k.size != 9:
        raise ValueError("K must have 9 entries")
    if dist is None:
        return k, None, k.ctypes.data_as(C.POINTER(C.c_double)), None
    d = np.ascontiguousarray(dist, np.float32).reshape(-1)
    if d.size != 5:
        raise ValueError("dist must be k1 k2 p1 p2 k3 (5 entries; pad k3 = 0)")
    return k, d, k.ctypes.data_as(C.POINTER(C.c_double)), d.ctypes.data_as(C.POINTER(C.c_float))


def _fisheye(K, K_raw, dist):
    """(K, K_raw [3,3] or [9] float64 -- K_raw None: K --, dist (k1, k2, k3, k4) float32 or None) -> the arrays (kept alive by the
    caller) and the three pointers the fisheye calls take."""
    if K is None and dist is None:
        return (None, None, None), (None, None, None)
    k = np.ascontiguousarray(K, np.float64).reshape(-1)
    kr = None if K_raw is None else np.ascontiguousarray(K_raw, np.float64).reshape(-1)
    if k.size != 9 or (kr is not None and kr.size != 9):
        raise ValueError("K and K_raw must have 9 entries")
    d = None if dist is None else np.ascontiguousarray(dist, np.float32).reshape(-1)
    if d is not None and d.size != 4:
        raise ValueError("dist must be k1 k2 k3 k4 (4 entries)")
    dp = C.POINTER(C.c_double)
    return (k, kr, d), (k.ctypes.data_as(dp), None if kr is None else kr.ctypes.data_as(dp),
                        None if d is None else d.ctypes.data_as(C.POINTER(C.c_float)))


def _dev_mask(t, ndim, what):
    """A device mask tensor: uint8 or bool (the same bytes: nonzero = the pixel takes part), contiguous."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what} must be a device (HIP) torch tensor; the NMI path has no CPU implementation")
    if t.dtype not in (torch.uint8, torch.bool) or t.dim() != ndim or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous uint8 or bool tensor with {ndim} dims, got {t.dtype} {tuple(t.shape)}")
    return t


def _dev_u8(t, ndim, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what} must be a device (HIP) torch tensor; the NMI path has no CPU implementation")
    if t.dtype != torch.uint8 or t.dim() != ndim or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous uint8 tensor with {ndim} dims, got {t.dtype} {tuple(t.shape)}")
    return t


class NmiContext:
    """nmi_ctx wrapper.  Mirrors the per-search objects of the reference (NmiObjects' buffers +
    the CUDA scratch of kernel.cu:59-73) as one persistent workspace."""

    # {option: value} applied to every new context (tests use it to run whole suites with one kernel selection)
    default_options = {}

    def __init__(self, width, height, bins=256, mode=MODE_SUC, use_bg=True, render_bottom_up=True, device=None,
                 stream=None, max_candidates=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: orbslam2_nmi_amd needs an AMD GPU (gfx950)")
        self._lib = load_library()
        self.width, self.height = int(width), int(height)
        self.bins, self.mode, self.use_bg, self.render_bottom_up = bins, mode, bool(use_bg), bool(render_bottom_up)
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", int(device) if not isinstance(device, torch.device) else device.index or 0)
        p = NmiParams()
        self._check(self._lib.nmi_params_default(C.byref(p), self.width, self.height), "nmi_params_default")
        p.bins, p.mode, p.use_bg, p.render_bottom_up = int(bins), int(mode), int(bool(use_bg)), int(bool(render_bottom_up))
        p.device = self.device.index
        p.max_candidates = int(max_candidates)
        p.stream = stream
        self._h = C.c_void_p()
        rc = self._lib.nmi_create(C.byref(p), C.byref(self._h))
        if rc != NMI_OK:
            self._h = C.c_void_p()
            raise NmiError(rc, "nmi_create")
        for opt, val in type(self).default_options.items():
            self.set_option(opt, val)

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != NMI_OK:
            detail = self._lib.nmi_last_error_detail(self._h).decode() if getattr(self, "_h", None) else ""
            raise NmiError(rc, what, detail)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nmi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream_handle):
        """Run on this hipStream_t (e.g. torch.cuda.Stream().cuda_stream); None = the context's own stream.

        The legacy default stream has handle 0, which the C ABI reads as "own stream": callers that need stream
        ordering with torch work (collectives, tensor reads) must make a non-default torch stream current and pass it."""
        if stream_handle == 0:
            raise ValueError("handle 0 is the legacy default stream; use a torch.cuda.Stream() (non-default) instead")
        self._check(self._lib.nmi_set_stream(self._h, C.c_void_p(stream_handle)), "nmi_set_stream")
        self._bound_stream = stream_handle

    def _order_after_torch(self):
        """Inputs produced by torch ops must be complete before this context's stream reads them: nothing to do when
        the context runs on torch's current stream, otherwise wait for that stream."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, "_bound_stream", None) != cur.cuda_stream:
            cur.synchronize()

    OPT_HIST_VARIANT, OPT_PHASE_MASK, OPT_WORKGROUPS, OPT_RESULT_PATH, OPT_XCD_TILING, OPT_TILE_QUEUE = 1, 2, 3, 4, 5, 6
    OPT_SPLIT, OPT_WAIT_MODE, OPT_STAMPS, OPT_SPLIT_PIXELS, OPT_CLIP_QUEUE = 7, 8, 9, 10, 11
    OPT_PIX_OWNER_BIAS = 14
    OPT_STAMP_CANDIDATE, OPT_WAVE_SHARES = 15, 16
    OPT_CONTENT_PATH, OPT_FEWLEVELS_BINS = 12, 13

    def set_option(self, option, value):
        self._check(self._lib.nmi_set_option(self._h, int(option), int(value)), "nmi_set_option")

    def synchronize(self):
        self._check(self._lib.nmi_synchronize(self._h), "nmi_synchronize")

    def set_profiling(self, on):
        self._check(self._lib.nmi_set_profiling(self._h, int(bool(on))), "nmi_set_profiling")

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(self._lib.nmi_last_kernel_ms(self._h, C.byref(ms)), "nmi_last_kernel_ms")
        return float(ms.value)

    def info(self):
        cu, wg, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.nmi_get_info(self._h, C.byref(cu), C.byref(wg), C.byref(lds)), "nmi_get_info")
        return {"compute_units": cu.value, "workgroups_per_launch": wg.value, "lds_bytes": lds.value}

    def last_content(self):
        """How the most recent search was scored -> {"few_levels": bool, "nr": int, "nw": int} (see nmi_last_content)."""
        f, r, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.nmi_last_content(self._h, C.byref(f), C.byref(r), C.byref(w)), "nmi_last_content")
        return {"few_levels": bool(f.value), "nr": r.value, "nw": w.value}

    def split_status(self):
        """Split-kernel liveness -> {"timeouts", "cooldown_calls_left", "next_cooldown", "last_launch_parts"} (nmi_split_status)."""
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self._lib.nmi_split_status(self._h, *[C.byref(x) for x in v]), "nmi_split_status")
        return dict(zip(("timeouts", "cooldown_calls_left", "next_cooldown", "last_launch_parts"), (x.value for x in v)))

    def pix_status(self):
        """Pixel-range kernel for mid-size grids -> {"last_launch_ranges", "healed"} (nmi_pix_status; waits for the stream)."""
        v = [C.c_int32(0) for _ in range(2)]
        self._check(self._lib.nmi_pix_status(self._h, *[C.byref(x) for x in v]), "nmi_pix_status")
        return dict(zip(("last_launch_ranges", "healed"), (x.value for x in v)))

    def pix_heal_counts(self):
        """Why the pixel-range kernels scored candidates once more, so far on this context -> {"timeouts", "count_test"}
        (nmi_pix_heal_counts; waits for the stream)."""
        v = [C.c_int32(0) for _ in range(2)]
        self._check(self._lib.nmi_pix_heal_counts(self._h, *[C.byref(x) for x in v]), "nmi_pix_heal_counts")
        return dict(zip(("timeouts", "count_test"), (x.value for x in v)))

    def term_table(self):
        """The per-count entropy-term table (NMI.cu:242-263 evaluated once per possible count) as numpy float32 [W*H+1]."""
        out = np.zeros(self.width * self.height + 1, np.float32)
        self._check(self._lib.nmi_copy_term_table(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                    "nmi_copy_term_table")
        return out

    def _img(self, t, what):
        t = _dev_u8(t, 2, what)
        if tuple(t.shape) != (self.height, self.width):
            raise ValueError(f"{what} is {tuple(t.shape)}, context is {(self.height, self.width)}")
        return t

    def _stack(self, t, what):
        t = _dev_u8(t, 3, what)
        if tuple(t.shape[1:]) != (self.height, self.width):
            raise ValueError(f"{what} is {tuple(t.shape)}, context images are {(self.height, self.width)}")
        return t

    # -- the path -------------------------------------------------------------------------------
    def eval_pair(self, render, warped):
        """CUDAF::NMIWithCuda_noMask (kernel.cu:49-114) for one (render, warped frame) pair -> float32 score."""
        r, w = self._img(render, "render"), self._img(warped, "warped")
        out = C.c_float(0)
        self._order_after_torch()
        self._check(self._lib.nmi_eval_pair(self._h, r.data_ptr(), w.data_ptr(), C.byref(out)), "nmi_eval_pair")
        return np.float32(out.value)

    def eval_pairs(self, renders, warps):
        """n independent (render, warped) pairs (lists of device images) in as few launches as possible -> float32 [n]."""
        assert len(renders) == len(warps)
        n = len(renders)
        rp = (C.c_void_p * max(n, 1))(*[self._img(r, "render").data_ptr() for r in renders])
        wp = (C.c_void_p * max(n, 1))(*[self._img(w, "warped").data_ptr() for w in warps])
        out = np.zeros(n, np.float32)
        self._order_after_torch()
        self._check(self._lib.nmi_eval_pairs(self._h, rp, wp, n, out.ctypes.data_as(C.POINTER(C.c_float))), "nmi_eval_pairs")
        return out

    def eval_pair_debug(self, render, warped):
        """-> (score, joint[256,256] u32 (render x warped), hist_render[256], hist_warped[256], sums[3]) as numpy."""
        import torch
        r, w = self._img(render, "render"), self._img(warped, "warped")
        joint = torch.zeros(65536, dtype=torch.int32, device=self.device)
        h1 = torch.zeros(256, dtype=torch.int32, device=self.device)
        h2 = torch.zeros(256, dtype=torch.int32, device=self.device)
        sums = torch.zeros(3, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        out = C.c_float(0)
        self._check(self._lib.nmi_eval_pair_debug(self._h, r.data_ptr(), w.data_ptr(), C.byref(out), joint.data_ptr(),
                                                  h1.data_ptr(), h2.data_ptr(), sums.data_ptr()), "nmi_eval_pair_debug")
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        return np.float32(out.value), u32(joint).reshape(256, 256), u32(h1), u32(h2), sums.cpu().numpy()

    def sort_points(self, xyz, red):
        """Point cloud (device float32 [N,3], [N]) -> copies in Morton order (nmi_sort_points): same renders, faster."""
        import torch
        assert xyz.is_cuda and red.is_cuda and xyz.dtype == torch.float32 and red.dtype == torch.float32
        xyz, red = xyz.contiguous(), red.contiguous()
        n = xyz.shape[0]
        assert tuple(xyz.shape) == (n, 3) and red.numel() == n
        xo, ro = torch.empty_like(xyz), torch.empty_like(red)
        self._order_after_torch()
        self._check(self._lib.nmi_sort_points(self._h, xyz.data_ptr(), red.data_ptr(), n, xo.data_ptr(), ro.data_ptr()), "nmi_sort_points")
        return xo, ro

    def sort_triangles(self, xyz, uv):
        """Triangle soup (device float32 [3T,3] corners, [3T,2] texture coordinates) -> copies in Morton order of the centroids."""
        import torch
        assert xyz.is_cuda and uv.is_cuda and xyz.dtype == torch.float32 and uv.dtype == torch.float32
        xyz, uv = xyz.contiguous(), uv.contiguous()
        t = xyz.shape[0] // 3
        assert tuple(xyz.shape) == (3 * t, 3) and tuple(uv.shape) == (3 * t, 2)
        xo, uo = torch.empty_like(xyz), torch.empty_like(uv)
        self._order_after_torch()
        self._check(self._lib.nmi_sort_triangles(self._h, xyz.data_ptr(), uv.data_ptr(), t, xo.data_ptr(), uo.data_ptr()), "nmi_sort_triangles")
        return xo, uo

    def sort_triangles_colored(self, xyz, red):
        """sort_triangles for a vertex-coloured mesh (device float32 [3T,3] corners, [3T] colours) -> copies in Morton order of the
        centroids; a triangle's three colours travel with its corners."""
        import torch
        assert xyz.is_cuda and red.is_cuda and xyz.dtype == torch.float32 and red.dtype == torch.float32
        xyz, red = xyz.contiguous(), red.contiguous()
        t = xyz.shape[0] // 3
        assert tuple(xyz.shape) == (3 * t, 3) and tuple(red.shape) == (3 * t,)
        xo, ro = torch.empty_like(xyz), torch.empty_like(red)
        self._order_after_torch()
        self._check(self._lib.nmi_sort_triangles_colored(self._h, xyz.data_ptr(), red.data_ptr(), t, xo.data_ptr(), ro.data_ptr()),
                    "nmi_sort_triangles_colored")
        return xo, ro

    def warp_stack(self, frame, homographies, out=None, sync=True):
        """Image::calculateWarping (image.cpp:115-128) on the device: frame [H,W] u8 + forward homographies [Wn,3,3]
        (float64, host) -> warp stack [Wn,H,W] u8 (device).  Enqueued on the context's stream."""
        import torch
        f = self._img(frame, "frame")
        m = np.ascontiguousarray(homographies, np.float64).reshape(-1, 9)
        wn = m.shape[0]
        if out is None:
            out = torch.empty((wn, self.height, self.width), dtype=torch.uint8, device=self.device)
        o = self._stack(out, "out")
        if o.shape[0] != wn:
            raise ValueError("out has the wrong number of warps")
        self._order_after_torch()  # `out` / `frame` may come from torch's stream
        self._check(self._lib.nmi_warp_stack(self._h, f.data_ptr(), m.ctypes.data_as(C.POINTER(C.c_double)), wn,
                                             o.data_ptr()), "nmi_warp_stack")
        if sync:
            self.synchronize()
        return out

    def warp_stack_masked(self, frame, homographies, frame_mask=None, out=None, out_masks=None, sync=True):
        """warp_stack plus the masks of its valid pixels (nmi_warp_stack_masked) -> (warps [Wn,H,W] u8, masks [Wn,H,W]).

        frame_mask: optional device [H,W] uint8 / bool, nonzero = usable frame pixel.  out_masks may be uint8 or bool (default
        uint8); mask bytes are 1 for a valid pixel, 0 otherwise.  The warps are byte-identical to warp_stack's."""
        import torch
        f = self._img(frame, "frame")
        m = np.ascontiguousarray(homographies, np.float64).reshape(-1, 9)
        wn = m.shape[0]
        fm = None
        if frame_mask is not None:
            fm = _dev_mask(frame_mask, 2, "frame_mask")
            if tuple(fm.shape) != (self.height, self.width):
                raise ValueError(f"frame_mask is {tuple(fm.shape)}, context is {(self.height, self.width)}")
        if out is None:
            out = torch.empty((wn, self.height, self.width), dtype=torch.uint8, device=self.device)
        if out_masks is None:
            out_masks = torch.empty((wn, self.height, self.width), dtype=torch.uint8, device=self.device)
        o, om = self._stack(out, "out"), self._mask_stack(out_masks, "out_masks")
        if o.shape[0] != wn or om.shape[0] != wn:
            raise ValueError("out / out_masks have the wrong number of warps")
        self._order_after_torch()
        self._check(self._lib.nmi_warp_stack_masked(self._h, f.data_ptr(), fm.data_ptr() if fm is not None else None,
                                                    m.ctypes.data_as(C.POINTER(C.c_double)), wn, o.data_ptr(), om.data_ptr()),
                    "nmi_warp_stack_masked")
        if sync:
            self.synchronize()
        return out, out_masks

    def undistort_frame(self, raw, K, dist, raw_mask=None, out=None, out_mask=None, sync=True):
        """nmi_undistort_frame: the raw camera frame [H,W] u8 (device) resampled onto the pinhole camera K ([3,3] float64) for the
        lens coefficients dist = (k1, k2, p1, p2, k3) -> (frame [H,W] u8, mask [H,W] u8 or None).  raw_mask: optional device
        [H,W] uint8 / bool, nonzero = usable raw pixel.  out_mask=False: no mask is written (None is returned in its place);
        otherwise a new uint8 tensor when None.  Enqueued on the context's stream."""
        k, d, kp, dp = _lens(K, dist)
        if d is None:
            raise ValueError("undistort_frame needs the five coefficients")
        return self._undistort(lambda *bufs: self._lib.nmi_undistort_frame(self._h, kp, dp, *bufs), "nmi_undistort_frame", raw, raw_mask,
                               out, out_mask, sync)

    def undistort_frame_fisheye(self, raw, K, K_raw, dist, raw_mask=None, out=None, out_mask=None, sync=True):
        """nmi_undistort_frame_fisheye: undistort_frame for the equidistant fisheye model (Kannala-Brandt): K ([3,3] float64) is the
        pinhole camera of the output, K_raw the camera the coefficients dist = (k1, k2, k3, k4) were calibrated with (None: K)."""
        keep, (kp, krp, dp) = _fisheye(K, K_raw, dist)
        if dp is None:
            raise ValueError("undistort_frame_fisheye needs the four coefficients")
        return self._undistort(lambda *bufs: self._lib.nmi_undistort_frame_fisheye(self._h, kp, krp, dp, *bufs), "nmi_undistort_frame_fisheye",
                               raw, raw_mask, out, out_mask, sync)

    def _undistort(self, call, what, raw, raw_mask, out, out_mask, sync):
        """The buffers of undistort_frame / undistort_frame_fisheye; call(raw, raw_mask, out, out_mask pointers) -> the C call's code."""
        import torch
        r = self._img(raw, "raw")
        rm = None
        if raw_mask is not None:
            rm = _dev_mask(raw_mask, 2, "raw_mask")
            if tuple(rm.shape) != (self.height, self.width):
                raise ValueError(f"raw_mask is {tuple(rm.shape)}, context is {(self.height, self.width)}")
        if out is None:
            out = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        o = self._img(out, "out")
        om = None
        if out_mask is None:
            out_mask = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        if out_mask is not False:
            om = _dev_mask(out_mask, 2, "out_mask")
            if tuple(om.shape) != (self.height, self.width):
                raise ValueError(f"out_mask is {tuple(om.shape)}, context is {(self.height, self.width)}")
        self._order_after_torch()
        self._check(call(r.data_ptr(), rm.data_ptr() if rm is not None else None, o.data_ptr(), om.data_ptr() if om is not None else None), what)
        if sync:
            self.synchronize()
        return out, om

    def gray_frame(self, src, fmt, pitch=0, out=None, sync=True):
        """nmi_gray_frame: the camera frame src (device uint8 tensor holding H rows of `pitch` bytes in format fmt, FRAME_*; pitch 0
        = dense, W * bytes per pixel) -> its dense grey frame [H,W] u8 (a new tensor when out is None).  src may be any uint8 tensor
        (a view whose first element is the frame's first byte) with at least (H - 1) * pitch + W * bytes per pixel bytes from there
        on.  Enqueued on the context's stream."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        need = _frame_bytes(fmt, pitch, self.width, self.height)
        if need is not None:
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        if out is None:
            out = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        o = self._img(out, "out")
        self._order_after_torch()
        self._check(self._lib.nmi_gray_frame(self._h, src.data_ptr(), int(fmt), int(pitch), o.data_ptr()), "nmi_gray_frame")
        if sync:
            self.synchronize()
        return out

    def set_tone_map(self, tm=None):
        """nmi_set_tone_map: the tone map (ToneMap; None: SHIFT, 16 bits) gray_frame, reduce_frame, tone_lut and tone_tile_luts
        apply to a FRAME_GRAY16 source from now on.  Ignored for every other format."""
        self._check(self._lib.nmi_set_tone_map(self._h, _tone_ref(tm)), "nmi_set_tone_map")
        self._tone = tm  # (a TABLE's tensor stays alive)

    def set_valid_range(self, lo=0, hi=65535):
        """nmi_set_valid_range: a FRAME_GRAY16 pixel is valid iff lo <= raw <= hi.  Invalid pixels stay out of the tone map's
        statistics (gray_frame, reduce_frame, tone_lut, tone_tile_luts, deep_frame) and are 0 in deep_frame's mask.  (0, 65535):
        off.  Ignored for every other format."""
        self._check(self._lib.nmi_set_valid_range(self._h, int(lo), int(hi)), "nmi_set_valid_range")

    def deep_frame(self, src, factor=1, pitch=0, frame_mask=None, out=None, out_mask=None, sync=True):
        """nmi_deep_frame: the FRAME_GRAY16 frame src (factor * H rows of `pitch` bytes, factor * W pixels each; src as for
        gray_frame) under the context's tone map and valid range -> (its grey frame [H,W] u8, its validity mask [H,W] u8: 1 where
        all factor x factor source pixels are valid and frame_mask -- optional device [H,W] uint8 / bool -- is nonzero).  New
        tensors when out / out_mask are None.  Enqueued on the context's stream."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        f = int(factor)
        if int(pitch) >= 0 and 1 <= f <= 4:
            need = (f * self.height - 1) * (int(pitch) or f * self.width * 2) + f * self.width * 2
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        fm = None
        if frame_mask is not None:
            fm = _dev_mask(frame_mask, 2, "frame_mask")
            if tuple(fm.shape) != (self.height, self.width):
                raise ValueError(f"frame_mask is {tuple(fm.shape)}, the search size is {(self.height, self.width)}")
        if out is None:
            out = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        if out_mask is None:
            out_mask = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        o, om = self._img(out, "out"), self._img(out_mask, "out_mask")
        self._order_after_torch()
        self._check(self._lib.nmi_deep_frame(self._h, src.data_ptr(), int(pitch), f, fm.data_ptr() if fm is not None else None, o.data_ptr(),
                                             om.data_ptr()), "nmi_deep_frame")
        if sync:
            self.synchronize()
        return out, out_mask

    def unpack_frame(self, src, fmt, factor=1, pitch=0, out=None, sync=True):
        """nmi_unpack_frame: the packed, big-endian or 16-bit mosaic deep frame src (factor * H rows of `pitch` bytes, factor * W
        pixels each in format fmt, one of FRAME_UNPACKED; src as for gray_frame) -> its dense FRAME_GRAY16 container, a device
        int16 tensor [factor*H, factor*W] holding the uint16 pixels' bits (view(torch.uint8) is what tone_lut, tone_tile_luts and
        deep_frame take).  A new tensor when out is None.  Enqueued on the context's stream."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        f = int(factor)
        shape = (f * self.height, f * self.width)
        need = _frame_bytes(fmt, pitch, shape[1], shape[0]) if 1 <= f <= 4 else None
        if need is not None:
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        if out is None:
            out = torch.empty(shape if 1 <= f <= 4 else (self.height, self.width), dtype=torch.int16, device=self.device)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int16 and out.is_contiguous()):
            raise TypeError("out must be a contiguous device int16 tensor")
        if 1 <= f <= 4 and tuple(out.shape) != shape:
            raise ValueError(f"out is {tuple(out.shape)}, the container is {shape}")
        self._order_after_torch()
        self._check(self._lib.nmi_unpack_frame(self._h, src.data_ptr(), int(fmt), int(pitch), f, out.data_ptr()), "nmi_unpack_frame")
        if sync:
            self.synchronize()
        return out

    def tone_lut(self, src, factor=1, pitch=0, out=None, window=True):
        """nmi_tone_lut: the uint8 table [TONE_LEVELS] the context's tone map gives for the FRAME_GRAY16 frame src (factor * H rows
        of `pitch` bytes, factor * W pixels each; src as for gray_frame).  window: blocks and returns (table, (lo, hi)); else the
        table alone, enqueued."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        f = int(factor)
        if int(pitch) >= 0 and 1 <= f <= 4:
            need = (f * self.height - 1) * (int(pitch) or f * self.width * 2) + f * self.width * 2
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        if out is None:
            out = torch.empty(TONE_LEVELS, dtype=torch.uint8, device=self.device)
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == TONE_LEVELS):
            raise TypeError(f"out must be a contiguous device uint8 tensor of {TONE_LEVELS} entries")
        pair = (C.c_int32 * 2)()
        self._order_after_torch()
        self._check(self._lib.nmi_tone_lut(self._h, src.data_ptr(), int(pitch), f, out.data_ptr(), pair if window else None), "nmi_tone_lut")
        return (out, (int(pair[0]), int(pair[1]))) if window else out

    def tone_tile_luts(self, src, factor=1, pitch=0, out=None, counts=True):
        """nmi_tone_tile_luts: the uint8 tables [tiles_y, tiles_x, TONE_LEVELS] the context's CLAHE tone map gives for the tiles of
        the FRAME_GRAY16 frame src (as for tone_lut).  counts: blocks and returns (tables, int32 [tiles_y, tiles_x] pixels per
        tile); else the tables alone, enqueued.  out: any contiguous device uint8 tensor of that many bytes."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        tm = getattr(self, "_tone", None)
        ty, tx = (tm.tiles_y, tm.tiles_x) if tm is not None and tm.mode == TONE_CLAHE else (1, 1)  # (else the call refuses)
        f = int(factor)
        if int(pitch) >= 0 and 1 <= f <= 4:
            need = (f * self.height - 1) * (int(pitch) or f * self.width * 2) + f * self.width * 2
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        if out is None:
            out = torch.empty((ty, tx, TONE_LEVELS), dtype=torch.uint8, device=self.device)
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == ty * tx * TONE_LEVELS):
            raise TypeError(f"out must be a contiguous device uint8 tensor of {ty * tx * TONE_LEVELS} entries")
        n = (C.c_int32 * (ty * tx))()
        self._order_after_torch()
        self._check(self._lib.nmi_tone_tile_luts(self._h, src.data_ptr(), int(pitch), f, out.data_ptr(), n if counts else None),
                    "nmi_tone_tile_luts")
        return (out, np.array(n, dtype=np.int32).reshape(ty, tx)) if counts else out

    def reduce_frame(self, src, fmt, factor, pitch=0, src_mask=None, out=None, out_mask=None, sync=True):
        """nmi_reduce_frame: the full-size camera frame src (device uint8 tensor holding factor * H rows of `pitch` bytes, each
        factor * W pixels in format fmt, FRAME_*; pitch 0 = dense) -> its grey frame at the context's size [H,W] u8: every pixel
        the rounded box average of factor x factor grey values.  src as for gray_frame, with at least (factor * H - 1) * pitch +
        factor * W * bytes per pixel bytes.  src_mask: optional device [factor*H, factor*W] uint8 / bool, nonzero = usable; then
        (frame, mask [H,W] u8: 1 where the whole block is usable) is returned, else the frame alone.  New tensors when out /
        out_mask are None.  Enqueued on the context's stream."""
        import torch
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8):
            raise TypeError("src must be a device uint8 tensor")
        f = int(factor)
        need = _frame_bytes(fmt, pitch, f * self.width, f * self.height) if 1 <= f <= 4 else None
        if need is not None:
            avail = src.untyped_storage().nbytes() - src.storage_offset()
            if avail < need:
                raise ValueError(f"src holds {avail} bytes from its first element, the frame needs {need}")
        sm = om = None
        if src_mask is not None:
            sm = _dev_mask(src_mask, 2, "src_mask")
            if 1 <= f <= 4 and tuple(sm.shape) != (f * self.height, f * self.width):
                raise ValueError(f"src_mask is {tuple(sm.shape)}, the full-size frame is {(f * self.height, f * self.width)}")
            if out_mask is None:
                out_mask = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
            om = self._img(out_mask, "out_mask")
        elif out_mask is not None:
            raise ValueError("out_mask goes with a src_mask")
        if out is None:
            out = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        o = self._img(out, "out")
        self._order_after_torch()
        self._check(self._lib.nmi_reduce_frame(self._h, src.data_ptr(), int(fmt), int(pitch), f, sm.data_ptr() if sm is not None else None,
                                               o.data_ptr(), om.data_ptr() if om is not None else None), "nmi_reduce_frame")
        if sync:
            self.synchronize()
        return out if sm is None else (out, out_mask)

    def _mask_stack(self, t, what):
        t = _dev_mask(t, 3, what)
        if tuple(t.shape[1:]) != (self.height, self.width):
            raise ValueError(f"{what} is {tuple(t.shape)}, context images are {(self.height, self.width)}")
        return t

    def search_grid_masked(self, render_stack, warp_stack, warp_masks, ratings=None):
        """search_grid with per-warp pixel masks (nmi_search_grid_masked) -> (best linear index w*S+s, best score).

        warp_masks: device [Wn,H,W] uint8 or bool, nonzero = the pixel takes part; ratings as for search_grid."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        wm = self._mask_stack(warp_masks, "warp_masks")
        S, Wn = rs.shape[0], ws.shape[0]
        if wm.shape[0] != Wn:
            raise ValueError(f"warp_masks has {wm.shape[0]} warps, warp_stack {Wn}")
        rp = self._ratings_ptr(ratings, Wn, S)
        idx, sc = C.c_int64(0), C.c_float(0)
        self._order_after_torch()
        self._check(self._lib.nmi_search_grid_masked(self._h, rs.data_ptr(), S, ws.data_ptr(), wm.data_ptr(), Wn, rp, C.byref(idx),
                                                     C.byref(sc)), "nmi_search_grid_masked")
        return int(idx.value), np.float32(sc.value)

    def mask_counts(self, n):
        """len_w (pixels taking part) of the first n warps of the latest masked search -> numpy int32 [n]."""
        out = np.zeros(int(n), np.int32)
        self._check(self._lib.nmi_last_mask_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), int(n)), "nmi_last_mask_counts")
        return out

    def search_grid_covered(self, render_stack, render_masks, warp_stack, warp_masks, ratings=None):
        """search_grid with masks on both sides (nmi_search_grid_covered) -> (best linear index w*S+s, best score).

        render_masks: device [S,H,W] uint8 or bool in the render's own layout (bottom-up rows like the render stack), nonzero =
        the map covers the pixel; warp_masks as for search_grid_masked; ratings as for search_grid."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        rm, wm = self._mask_stack(render_masks, "render_masks"), self._mask_stack(warp_masks, "warp_masks")
        S, Wn = rs.shape[0], ws.shape[0]
        if rm.shape[0] != S:
            raise ValueError(f"render_masks has {rm.shape[0]} renders, render_stack {S}")
        if wm.shape[0] != Wn:
            raise ValueError(f"warp_masks has {wm.shape[0]} warps, warp_stack {Wn}")
        rp = self._ratings_ptr(ratings, Wn, S)
        idx, sc = C.c_int64(0), C.c_float(0)
        self._order_after_torch()
        self._check(self._lib.nmi_search_grid_covered(self._h, rs.data_ptr(), rm.data_ptr(), S, ws.data_ptr(), wm.data_ptr(), Wn, rp,
                                                      C.byref(idx), C.byref(sc)), "nmi_search_grid_covered")
        return int(idx.value), np.float32(sc.value)

    def cover_counts(self, n):
        """len[w][s] (pixels where both masks are nonzero) of the first n candidates of the latest covered search, layout
        [Wn][S] flattened -> numpy int32 [n]."""
        out = np.zeros(int(n), np.int32)
        self._check(self._lib.nmi_last_cover_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), int(n)), "nmi_last_cover_counts")
        return out

    def pack_mask_bits(self, masks, out=None, sync=True):
        """Bit-pack device masks [n,H,W] (uint8 / bool, nonzero = set) -> device uint8 [n, ceil(H*W/8)] (nmi_pack_mask_bits):
        pixel p of image i is bit p % 8 (LSB first) of byte p // 8 of row i, as np.packbits(..., bitorder="little").  The form in
        which NmiStream.submit_covered takes render masks."""
        import torch
        m = self._mask_stack(masks, "masks")
        n, nb = m.shape[0], (self.width * self.height + 7) // 8
        if out is None:
            out = torch.empty((n, nb), dtype=torch.uint8, device=self.device)
        o = _dev_u8(out, 2, "out")
        if tuple(o.shape) != (n, nb):
            raise ValueError(f"out is {tuple(o.shape)}, bits need {(n, nb)}")
        self._order_after_torch()
        self._check(self._lib.nmi_pack_mask_bits(self._h, m.data_ptr(), n, o.data_ptr()), "nmi_pack_mask_bits")
        if sync:
            self.synchronize()
        return out

    def _new_stack(self, S, dtype=None):
        import torch
        return torch.empty((S, self.height, self.width), dtype=dtype or torch.uint8, device=self.device)

    def _out_masks(self, S, out_masks):
        """The out_masks stack of a masked render of S views: made if None, else checked -> (what the caller gets back, its bytes)."""
        if out_masks is None:
            out_masks = self._new_stack(S)
        om = self._mask_stack(out_masks, "out_masks")
        if om.shape[0] != S:
            raise ValueError("out_masks has the wrong number of views")
        return out_masks, om

    def _render(self, mvps, out, sync, call, name, masked=False, out_masks=None):
        """What the colour renders share: host MVPs as float32 [S,16], the render stack (made if None), with `masked` the masks stack,
        ordering after torch, and the C call -- call(S, mvps pointer, out pointer[, masks pointer]) -> status of the C function `name`.
        -> out, or (out, out_masks)."""
        m = np.ascontiguousarray(mvps, np.float32).reshape(-1, 16)
        S = m.shape[0]
        ptrs = ()
        if masked:
            out_masks, om = self._out_masks(S, out_masks)
            ptrs = (om.data_ptr(),)
        if out is None:
            out = self._new_stack(S)
        o = self._stack(out, "out")
        self._order_after_torch()
        self._check(call(S, m.ctypes.data_as(C.POINTER(C.c_float)), o.data_ptr(), *ptrs), name)
        if sync:
            self.synchronize()
        return (out, out_masks) if masked else out

    @staticmethod
    def _cloud_tensors(xyz, red):
        import torch
        for t, shape in ((xyz, 2), (red, 1)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != shape:
                raise TypeError("xyz must be a contiguous float32 device tensor [N,3], red one of [N]")

    @staticmethod
    def _mesh_tensors(xyz, uv):
        import torch
        for t, cols in ((xyz, 3), (uv, 2)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != cols:
                raise TypeError("xyz / uv must be contiguous float32 device tensors [3T,3] / [3T,2]")
        if xyz.shape[0] != uv.shape[0] or xyz.shape[0] % 3:
            raise ValueError("xyz and uv must hold three corners per triangle")

    @staticmethod
    def _colored_mesh_tensors(xyz, red):
        import torch
        for t, dims in ((xyz, 2), (red, 1)):
            if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != dims or (dims == 2 and t.shape[1] != 3):
                raise TypeError("xyz / red must be contiguous float32 device tensors [3T,3] / [3T]")
        if xyz.shape[0] != red.shape[0] or xyz.shape[0] % 3:
            raise ValueError("xyz and red must hold three corners per triangle")

    def render_points_masked(self, xyz, red, mvps, point_size, out=None, out_masks=None, sync=True):
        """render_points plus its coverage (nmi_render_points_masked) -> (renders [S,H,W] u8, masks [S,H,W]): mask bytes are 1
        where a point won the pixel, 0 where it kept the background; bottom-up rows like the renders, which are
        byte-identical to render_points'.  out_masks may be uint8 or bool (default uint8)."""
        self._cloud_tensors(xyz, red)
        return self._render(mvps, out, sync, lambda S, mp, o, om: self._lib.nmi_render_points_masked(
            self._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0], mp, S, float(point_size), o, om), "nmi_render_points_masked", True, out_masks)

    def render_mesh_masked(self, xyz, uv, texture, mvps, out=None, out_masks=None, sync=True):
        """render_mesh plus its coverage (nmi_render_mesh_masked) -> (renders [S,H,W] u8, masks [S,H,W]): mask bytes are 1
        where a triangle won the pixel, 0 where it kept the background; the renders are byte-identical to render_mesh's."""
        self._mesh_tensors(xyz, uv)
        return self._render(mvps, out, sync, lambda S, mp, o, om: self._lib.nmi_render_mesh_masked(
            self._h, xyz.data_ptr(), uv.data_ptr(), xyz.shape[0] // 3, texture._h, mp, S, o, om), "nmi_render_mesh_masked", True, out_masks)

    def render_points(self, xyz, red, mvps, point_size, out=None, sync=True):
        """Rendering<4>::renderToTextureOnGPU without OpenGL: device float32 xyz [N,3] + red [N], host MVPs [S,16]
        (render_mvp) -> render stack [S,H,W] u8 on the device, bottom-up rows, background 255."""
        self._cloud_tensors(xyz, red)
        return self._render(mvps, out, sync, lambda S, mp, o: self._lib.nmi_render_points(
            self._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0], mp, S, float(point_size), o), "nmi_render_points")

    def render_mesh(self, xyz, uv, texture, mvps, out=None, sync=True):
        """Rendering<1>::renderToTextureOnGPU without OpenGL: device float32 corner arrays xyz [3T,3], uv [3T,2], an
        NmiTexture, host MVPs [S,16] -> render stack [S,H,W] u8 on the device (bottom-up rows, background 255)."""
        self._mesh_tensors(xyz, uv)
        return self._render(mvps, out, sync, lambda S, mp, o: self._lib.nmi_render_mesh(
            self._h, xyz.data_ptr(), uv.data_ptr(), xyz.shape[0] // 3, texture._h, mp, S, o), "nmi_render_mesh")

    def render_mesh_colored(self, xyz, red, mvps, out=None, sync=True):
        """A vertex-coloured mesh (nmi_render_mesh_colored): device float32 corner arrays xyz [3T,3] and red [3T] (one colour per
        corner, no texture), host MVPs [S,16] -> render stack [S,H,W] u8 on the device (bottom-up rows, background 255)."""
        self._colored_mesh_tensors(xyz, red)
        return self._render(mvps, out, sync, lambda S, mp, o: self._lib.nmi_render_mesh_colored(
            self._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0] // 3, mp, S, o), "nmi_render_mesh_colored")

    def render_mesh_colored_masked(self, xyz, red, mvps, out=None, out_masks=None, sync=True):
        """render_mesh_colored plus its coverage (nmi_render_mesh_colored_masked) -> (renders [S,H,W] u8, masks [S,H,W]), as
        render_mesh_masked."""
        self._colored_mesh_tensors(xyz, red)
        return self._render(mvps, out, sync, lambda S, mp, o, om: self._lib.nmi_render_mesh_colored_masked(
            self._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0] // 3, mp, S, o, om), "nmi_render_mesh_colored_masked", True, out_masks)

    def _depth_outputs(self, S, out, out_masks, depth16):
        """The three stacks of a depth render: grey (made if None), masks and raw depths (None, True = make one, or a tensor)."""
        import torch
        shape = (S, self.height, self.width)
        if out is None:
            out = self._new_stack(S)
        o = self._stack(out, "out")
        om = None
        if out_masks is not None:
            out_masks, om = self._out_masks(S, None if out_masks is True else out_masks)
        if depth16 is True:
            depth16 = self._new_stack(S, torch.int16)
        if depth16 is not None and not (depth16.is_cuda and depth16.element_size() == 2 and depth16.is_contiguous()
                                        and tuple(depth16.shape) == shape):
            raise TypeError(f"depth16 must be a contiguous 16-bit device tensor {shape}")
        return out, o, out_masks, om, depth16

    def render_points_depth(self, xyz, red, mvps, point_size, shade, out=None, out_masks=None, depth16=None, sync=True):
        """The depth render of a cloud (nmi_render_points_depth): xyz [N,3], red [N] or None (every point splats colour 0), host MVPs
        [S,16], an NmiDepthShade -> (grey [S,H,W] u8, masks or None, depth16 or None).  out_masks / depth16: None (not wanted),
        True (made here; depth16 as int16, the raw depths being its bits as uint16) or a tensor of the stack's shape."""
        import torch
        if not xyz.is_cuda or xyz.dtype != torch.float32 or not xyz.is_contiguous() or xyz.dim() != 2:
            raise TypeError("xyz must be a contiguous float32 device tensor [N,3]")
        if red is not None and (not red.is_cuda or red.dtype != torch.float32 or not red.is_contiguous() or red.dim() != 1):
            raise TypeError("red must be a contiguous float32 device tensor [N] or None")
        m = np.ascontiguousarray(mvps, np.float32).reshape(-1, 16)
        out, o, out_masks, om, depth16 = self._depth_outputs(m.shape[0], out, out_masks, depth16)
        self._order_after_torch()
        self._check(self._lib.nmi_render_points_depth(self._h, xyz.data_ptr(), red.data_ptr() if red is not None else None, xyz.shape[0],
                                                      m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], float(point_size), _shade_ref(shade),
                                                      o.data_ptr(), om.data_ptr() if om is not None else None,
                                                      depth16.data_ptr() if depth16 is not None else None), "nmi_render_points_depth")
        if sync:
            self.synchronize()
        return out, out_masks, depth16

    def render_mesh_depth(self, xyz, mvps, shade, out=None, out_masks=None, depth16=None, sync=True):
        """The depth render of a mesh (nmi_render_mesh_depth): corner positions xyz [3T,3] alone, host MVPs [S,16], an NmiDepthShade
        -> (grey [S,H,W] u8, masks or None, depth16 or None), as render_points_depth."""
        import torch
        if not xyz.is_cuda or xyz.dtype != torch.float32 or not xyz.is_contiguous() or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] % 3:
            raise TypeError("xyz must be a contiguous float32 device tensor [3T,3]")
        m = np.ascontiguousarray(mvps, np.float32).reshape(-1, 16)
        out, o, out_masks, om, depth16 = self._depth_outputs(m.shape[0], out, out_masks, depth16)
        self._order_after_torch()
        self._check(self._lib.nmi_render_mesh_depth(self._h, xyz.data_ptr(), xyz.shape[0] // 3, m.ctypes.data_as(C.POINTER(C.c_float)),
                                                    m.shape[0], _shade_ref(shade), o.data_ptr(), om.data_ptr() if om is not None else None,
                                                    depth16.data_ptr() if depth16 is not None else None), "nmi_render_mesh_depth")
        if sync:
            self.synchronize()
        return out, out_masks, depth16

    def depth_shade_apply(self, shade, depth24, sync=True):
        """The depth shade on an array (nmi_depth_shade_apply): depth24 a contiguous 32-bit integer device tensor of 24-bit window
        depths -> (v int16 tensor holding the raw depths' bits as uint16, grey uint8 tensor), both of depth24's shape."""
        import torch
        if not depth24.is_cuda or depth24.element_size() != 4 or depth24.is_floating_point() or not depth24.is_contiguous():
            raise TypeError("depth24 must be a contiguous 32-bit integer device tensor")
        v = torch.empty(depth24.shape, dtype=torch.int16, device=depth24.device)
        g = torch.empty(depth24.shape, dtype=torch.uint8, device=depth24.device)
        self._order_after_torch()
        self._check(self._lib.nmi_depth_shade_apply(self._h, _shade_ref(shade), depth24.data_ptr(), depth24.numel(), v.data_ptr(), g.data_ptr()),
                    "nmi_depth_shade_apply")
        if sync:
            self.synchronize()
        return v, g

    def search_grid(self, render_stack, warp_stack, ratings=None):
        """Candidate loop + arg-max (Tracking.cc:1879-1905,1952).  -> (best linear index w*S+s, best score).

        ratings: optional device float32 tensor [Wn, S] that receives the full rating table."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        S, Wn = rs.shape[0], ws.shape[0]
        rp = self._ratings_ptr(ratings, Wn, S)
        idx, sc = C.c_int64(0), C.c_float(0)
        self._order_after_torch()  # the stacks (and a pre-filled ratings tensor) may come from torch's stream
        self._check(self._lib.nmi_search_grid(self._h, rs.data_ptr(), S, ws.data_ptr(), Wn, rp, C.byref(idx), C.byref(sc)),
                    "nmi_search_grid")
        return int(idx.value), np.float32(sc.value)

    def bind_search(self, render_stack, warp_stack, ratings=None):
        """The arguments of search_grid converted ONCE -> a callable () -> (best linear index, best score) that makes the blocking
        nmi_search_grid call and nothing else.  For loops that repeat one search many times (bench.py's timed region): the checks
        and conversions of search_grid cost the interpreter a few microseconds per call, which is harness, not library.  The
        stacks must already be complete on the device (the caller synchronises once before the loop) and stay alive."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        S, Wn = rs.shape[0], ws.shape[0]
        rp = self._ratings_ptr(ratings, Wn, S)
        idx, sc = C.c_int64(0), C.c_float(0)
        pidx, psc, fn, handle = C.byref(idx), C.byref(sc), self._lib.nmi_search_grid, self._h
        prs, pws, cS, cWn = C.c_void_p(rs.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_int32(S), C.c_int32(Wn)
        prp = C.c_void_p(rp) if rp is not None else None
        check = self._check
        self._order_after_torch()

        def call(_keep=(rs, ws, ratings)):
            rc = fn(handle, prs, cS, pws, cWn, prp, pidx, psc)
            if rc != NMI_OK:
                check(rc, "nmi_search_grid")
            return idx.value, sc.value
        return call

    def search_grid_shard(self, render_stack, s_offset, s_total, warp_stack, ratings=None, key_out=None, blocking=True,
                          w_offset=0, wn_total=None):
        """One rank's part of a sharded search.  -> packed key (int) if blocking else None.

        key_out: optional device int64/uint64 tensor of one element that receives the key (for a collective).
        w_offset / wn_total: position of the given warps in the global warp axis when that axis is sharded too."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        S, Wn = rs.shape[0], ws.shape[0]
        rp = self._ratings_ptr(ratings, Wn, S)
        kp = None
        if key_out is not None:
            if not key_out.is_cuda or key_out.numel() != 1 or key_out.element_size() != 8:
                raise TypeError("key_out must be a one-element 64-bit device tensor")
            kp = key_out.data_ptr()
        hk = C.c_uint64(0)
        self._order_after_torch()
        self._check(self._lib.nmi_search_grid_block(self._h, rs.data_ptr(), S, int(s_offset), int(s_total), ws.data_ptr(),
                                                    Wn, int(w_offset), int(Wn + w_offset if wn_total is None else wn_total), rp, kp,
                                                    C.byref(hk) if blocking else None),
                    "nmi_search_grid_block")
        return int(hk.value) if blocking else None

    def rank_peaks(self, ratings, num, K, radius, keys_out=None, blocking=True):
        """nmi_rank_peaks: the K best separated candidates of a device rating table (include/nmi_hip.h, "Ranked peaks").
        ratings: contiguous float32 device tensor of prod(num) cells, [Wn, S] as search_grid fills it; num, radius: six ints each
        (axis order of nmi_host.h); K in 1 .. PEAKS_MAX_K.  keys_out: optional device int64 / uint64 tensor of K elements that
        receives the keys too.  blocking -> (keys uint64 [K] numpy, zeros after the peaks; count); else the call only enqueues
        (keys_out is then required) and returns None."""
        import torch
        if not isinstance(ratings, torch.Tensor) or not ratings.is_cuda or ratings.dtype != torch.float32 or not ratings.is_contiguous():
            raise TypeError("ratings must be a contiguous float32 device tensor")
        num6, rad6 = (C.c_int32 * 6)(*[int(v) for v in num]), (C.c_int32 * 6)(*[int(v) for v in radius])
        if all(v >= 1 for v in num6) and ratings.numel() != int(np.prod(list(num6), dtype=np.int64)):
            raise ValueError("ratings must have prod(num) cells")
        kp = None
        if keys_out is not None:
            if not keys_out.is_cuda or keys_out.numel() != int(K) or keys_out.element_size() != 8 or not keys_out.is_contiguous():
                raise TypeError("keys_out must be a contiguous 64-bit device tensor of K elements")
            kp = keys_out.data_ptr()
        keys, n = np.zeros(max(int(K), 1), np.uint64), C.c_int32(0)
        self._order_after_torch()
        self._check(self._lib.nmi_rank_peaks(self._h, ratings.data_ptr(), num6, int(K), rad6, kp,
                                             keys.ctypes.data_as(C.POINTER(C.c_uint64)) if blocking else None, C.byref(n)),
                    "nmi_rank_peaks")
        return (keys[:int(K)], int(n.value)) if blocking else None

    def bind_rank_peaks(self, ratings, num, K, radius):
        """The arguments of the blocking rank_peaks converted ONCE -> (call, keys): call() makes the nmi_rank_peaks call and nothing
        else and returns the count; keys (uint64 [K] numpy) receives every call's keys.  For loops that time the call
        (tools/peaks_time.py), as bind_search is for the search; the table must be complete on the context's stream."""
        num6, rad6 = (C.c_int32 * 6)(*[int(v) for v in num]), (C.c_int32 * 6)(*[int(v) for v in radius])
        keys, n = np.zeros(int(K), np.uint64), C.c_int32(0)
        fn, handle, check = self._lib.nmi_rank_peaks, self._h, self._check
        pr, pk, pn, cK = C.c_void_p(ratings.data_ptr()), keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), C.c_int32(int(K))
        self._order_after_torch()

        def call(_keep=(ratings, num6, rad6, keys)):
            rc = fn(handle, pr, num6, cK, rad6, None, pk, pn)
            if rc != NMI_OK:
                check(rc, "nmi_rank_peaks")
            return n.value
        return call, keys

    def refine_peaks(self, ratings, num, keys, records_out=None, blocking=True):
        """nmi_refine_peaks: sub-cell offset, interpolated score and Hessian of K peaks of a device rating table
        (include/nmi_hip.h, "Refined peaks").  ratings, num: as rank_peaks takes them.  keys: the K keys, 1 <= K <= PEAKS_MAX_K, as
        rank_peaks gives them -- a contiguous 64-bit device tensor (read in stream order) or a host sequence / uint64 array (they
        travel with the launch).  records_out: optional device uint8 tensor of K * 152 bytes that receives the records too.
        blocking -> REFINED_PEAK [K] numpy; else the call only enqueues (records_out is then required) and returns None."""
        import torch
        if not isinstance(ratings, torch.Tensor) or not ratings.is_cuda or ratings.dtype != torch.float32 or not ratings.is_contiguous():
            raise TypeError("ratings must be a contiguous float32 device tensor")
        num6 = (C.c_int32 * 6)(*[int(v) for v in num])
        if all(v >= 1 for v in num6) and ratings.numel() != int(np.prod(list(num6), dtype=np.int64)):
            raise ValueError("ratings must have prod(num) cells")
        dk = hk = None
        if isinstance(keys, torch.Tensor):
            if not keys.is_cuda or keys.element_size() != 8 or not keys.is_contiguous():
                raise TypeError("device keys must be a contiguous 64-bit device tensor")
            K, dk = keys.numel(), keys.data_ptr()
        else:
            host = np.ascontiguousarray(keys, np.uint64).reshape(-1)
            K, hk = host.size, host.ctypes.data_as(C.POINTER(C.c_uint64))
        op = None
        if records_out is not None:
            if (not records_out.is_cuda or records_out.dtype != torch.uint8 or records_out.numel() != K * REFINED_PEAK.itemsize
                    or not records_out.is_contiguous()):
                raise TypeError("records_out must be a contiguous uint8 device tensor of K * 152 bytes")
            op = records_out.data_ptr()
        records = np.zeros(max(K, 1), REFINED_PEAK)
        self._order_after_torch()
        self._check(self._lib.nmi_refine_peaks(self._h, ratings.data_ptr(), num6, dk, hk, K, op, records.ctypes.data if blocking else None),
                    "nmi_refine_peaks")
        return records[:K] if blocking else None

    def _ratings_ptr(self, ratings, Wn, S):
        import torch
        if ratings is None:
            return None
        if (not ratings.is_cuda or ratings.dtype != torch.float32 or not ratings.is_contiguous()
                or ratings.numel() != Wn * S):
            raise TypeError(f"ratings must be a contiguous float32 device tensor with {Wn * S} elements")
        return ratings.data_ptr()

    # -- RCCL -----------------------------------------------------------------------------------
    def rccl_comm_init(self, unique_id: bytes, rank, nranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        comm = C.c_void_p()
        self._check(self._lib.nmi_rccl_comm_init(self._h, buf, rank, nranks, C.byref(comm)), "nmi_rccl_comm_init")
        return comm

    def search_grid_rccl(self, render_stack, s_offset, s_total, warp_stack, comm, ratings=None, w_offset=0, wn_total=None):
        """One rank's block of a sharded search + the RCCL MAX all-reduce of the packed winner -> global (index, score)."""
        rs, ws = self._stack(render_stack, "render_stack"), self._stack(warp_stack, "warp_stack")
        S, Wn = rs.shape[0], ws.shape[0]
        idx, sc = C.c_int64(0), C.c_float(0)
        self._order_after_torch()
        self._check(self._lib.nmi_search_grid_block_rccl(self._h, rs.data_ptr(), S, int(s_offset), int(s_total), ws.data_ptr(),
                                                         Wn, int(w_offset), int(Wn + w_offset if wn_total is None else wn_total),
                                                         self._ratings_ptr(ratings, Wn, S), comm, C.byref(idx), C.byref(sc)),
                    "nmi_search_grid_block_rccl")
        return int(idx.value), np.float32(sc.value)


class NmiTexture:
    """nmi_texture wrapper: RGB8 image as handed to glTexImage2D -> mip chain -> per-level luma on the device."""

    def __init__(self, ctx, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.ndim == 3 and rgb.shape[2] == 3
        self.ctx, self._lib = ctx, ctx._lib
        self._h = C.c_void_p()
        ctx._check(self._lib.nmi_texture_create(ctx._h, rgb.ctypes.data_as(C.c_void_p), rgb.shape[1], rgb.shape[0],
                                                C.byref(self._h)), "nmi_texture_create")

    def close(self):
        if self._h and self._h.value:
            self._lib.nmi_texture_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class NmiLevel:
    """nmi_level wrapper: cloud + frame -> renders, warps, search, winner as one captured HIP graph."""

    def __init__(self, ctx, xyz, red, frame, S, Wn, point_size, texture=None, block=None, colors=False, depth=None, mesh=False):
        """Point cloud: xyz [N,3], red [N], point_size.  Textured mesh: pass texture=NmiTexture, xyz [3T,3] corner
        positions and `red` = uv [3T,2] (point_size is ignored).  Vertex-coloured mesh: colors=True, xyz [3T,3] and red [3T],
        no texture (point_size is ignored).
        block = (s_offset, S_total, w_offset, Wn_total): this level is one rank's block (S views x Wn warps, either may be 0)
        of a level sharded over ranks (nmi_level_create_block); winners then carry global indices.
        depth = NmiDepthShade with red=None: a depth level of a map without attributes (nmi_level_create_depth_block) -- a cloud
        xyz [N,3], or with mesh=True the corner positions xyz [3T,3] of a mesh.  (A level WITH attributes becomes a depth level
        through set_depth_shade.)"""
        self.ctx, self._lib = ctx, ctx._lib
        self._keep = (xyz, red, frame, texture)  # the graph holds their device addresses
        self.S, self.Wn = int(S), int(Wn)
        self._h = C.c_void_p()
        ctx._order_after_torch()
        if block is None:
            block = (0, self.S, 0, self.Wn)
        so, st, wo, wt = (int(v) for v in block)
        if depth is not None:
            if red is not None or texture is not None or colors:
                raise ValueError("a depth level is created without attributes; use set_depth_shade on a level that has them")
            self._shade = depth
            ctx._check(self._lib.nmi_level_create_depth_block(ctx._h, MAP_MESH if mesh else MAP_POINTS, xyz.data_ptr(),
                                                              xyz.shape[0] // 3 if mesh else xyz.shape[0], frame.data_ptr(), self.S, so, st,
                                                              self.Wn, wo, wt, float(point_size), _shade_ref(depth), C.byref(self._h)),
                       "nmi_level_create_depth_block")
        elif colors:
            if texture is not None:
                raise ValueError("a vertex-coloured mesh level takes no texture")
            ctx._check(self._lib.nmi_level_create_mesh_colored_block(ctx._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0] // 3,
                                                                     frame.data_ptr(), self.S, so, st, self.Wn, wo, wt, C.byref(self._h)),
                       "nmi_level_create_mesh_colored_block")
        elif texture is None:
            ctx._check(self._lib.nmi_level_create_block(ctx._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0], frame.data_ptr(), self.S, so,
                                                        st, self.Wn, wo, wt, float(point_size), C.byref(self._h)), "nmi_level_create_block")
        else:
            ctx._check(self._lib.nmi_level_create_mesh_block(ctx._h, xyz.data_ptr(), red.data_ptr(), xyz.shape[0] // 3, texture._h,
                                                             frame.data_ptr(), self.S, so, st, self.Wn, wo, wt, C.byref(self._h)),
                       "nmi_level_create_mesh_block")

    def _params(self, mvps, homographies):
        m = np.ascontiguousarray(mvps, np.float32).reshape(-1)
        h = np.ascontiguousarray(homographies, np.float64).reshape(-1)
        assert m.size == self.S * 16 and h.size == self.Wn * 9
        return m, h, (m.ctypes.data_as(C.POINTER(C.c_float)) if m.size else None), (h.ctypes.data_as(C.POINTER(C.c_double)) if h.size else None)

    def run(self, mvps, homographies):
        """mvps [S,16], homographies [Wn,3,3] of THIS block -> (global index, score) of the block's winner."""
        m, h, mp, hp = self._params(mvps, homographies)
        idx, sc = C.c_int64(0), C.c_float(0)
        self.ctx._check(self._lib.nmi_level_run(self._h, mp, hp, C.byref(idx), C.byref(sc)), "nmi_level_run")
        return int(idx.value), np.float32(sc.value)

    def bind(self, mvps, homographies, comm=None):
        """Parameters converted ONCE -> a callable that replays the level with them: () -> (global index, score).  For loops that
        replay a few fixed parameter sets many times (bench.py --config e2e): the conversions of run() cost the interpreter ~20 us a
        call, a tenth of the level."""
        m, h, mp, hp = self._params(mvps, homographies)
        idx, sc = C.c_int64(0), C.c_float(0)
        pidx, psc, lib, handle, check = C.byref(idx), C.byref(sc), self._lib, self._h, self.ctx._check

        def replay(_keep=(m, h)):   # (the arrays behind the pointers stay alive with the closure)
            if comm is None:
                check(lib.nmi_level_run(handle, mp, hp, pidx, psc), "nmi_level_run")
            else:
                check(lib.nmi_level_run_rccl(handle, mp, hp, comm, pidx, psc), "nmi_level_run_rccl")
            return idx.value, sc.value
        return replay

    def run_rccl(self, mvps, homographies, comm):
        """The same + the level's MAX all-reduce over the RCCL communicator -> the LEVEL's winner, on every rank."""
        m, h, mp, hp = self._params(mvps, homographies)
        idx, sc = C.c_int64(0), C.c_float(0)
        self.ctx._check(self._lib.nmi_level_run_rccl(self._h, mp, hp, comm, C.byref(idx), C.byref(sc)), "nmi_level_run_rccl")
        return int(idx.value), np.float32(sc.value)

    def outputs(self):
        """-> (renders [S,H,W] u8, warps [Wn,H,W] u8, ratings [Wn,S] f32) of the latest run, as numpy (host copies)."""
        h, w = self.ctx.height, self.ctx.width
        r = np.empty((self.S, h, w), np.uint8)
        v = np.empty((self.Wn, h, w), np.uint8)
        t = np.empty((self.Wn, self.S), np.float32)
        self.ctx._check(self._lib.nmi_level_copy_outputs(self._h, r.ctypes.data, v.ctypes.data, t.ctypes.data), "nmi_level_copy_outputs")
        return r, v, t

    def set_masks(self, enabled=True, frame_mask=None):
        """Masked level (nmi_level_set_masks): every replay also computes the warps' masks (border masks, and frame_mask where
        given) and scores with the masked search's arithmetic.  frame_mask: device [H,W] uint8 / bool, nonzero = usable, or None;
        the level reads it in place on every replay (its contents may change between runs) and keeps it alive.
        enabled=False restores the unmasked level."""
        fm = None
        if frame_mask is not None:
            if not enabled:
                raise ValueError("set_masks(enabled=False) takes no frame_mask")
            fm = _dev_mask(frame_mask, 2, "frame_mask")
            if tuple(fm.shape) != (self.ctx.height, self.ctx.width):
                raise ValueError(f"frame_mask is {tuple(fm.shape)}, context is {(self.ctx.height, self.ctx.width)}")
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_masks(self._h, int(bool(enabled)), fm.data_ptr() if fm is not None else None),
                        "nmi_level_set_masks")
        self._frame_mask = fm  # the graph holds its device address

    def masks(self):
        """-> (warp masks [Wn,H,W] u8, counts [Wn] int32) of the latest run of a masked level, as numpy (host copies)."""
        m = np.empty((self.Wn, self.ctx.height, self.ctx.width), np.uint8)
        n = np.empty(self.Wn, np.int32)
        self.ctx._check(self._lib.nmi_level_copy_masks(self._h, m.ctypes.data, n.ctypes.data_as(C.POINTER(C.c_int32))), "nmi_level_copy_masks")
        return m, n

    def set_coverage(self, enabled=True, frame_mask=None):
        """Covered level (nmi_level_set_coverage): every replay also writes the renders' coverage masks and the warps' masks
        (border masks, and frame_mask where given) and scores with the covered search's arithmetic (masks on both sides).
        frame_mask: device [H,W] uint8 / bool, nonzero = usable, or None; read in place on every replay and kept alive.
        enabled=False restores the unmasked level.  A masked level cannot be covered (set_masks(False) first), nor the reverse."""
        fm = None
        if frame_mask is not None:
            if not enabled:
                raise ValueError("set_coverage(enabled=False) takes no frame_mask")
            fm = _dev_mask(frame_mask, 2, "frame_mask")
            if tuple(fm.shape) != (self.ctx.height, self.ctx.width):
                raise ValueError(f"frame_mask is {tuple(fm.shape)}, context is {(self.ctx.height, self.ctx.width)}")
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_coverage(self._h, int(bool(enabled)), fm.data_ptr() if fm is not None else None),
                        "nmi_level_set_coverage")
        self._frame_mask = fm  # the graph holds its device address

    def coverage(self):
        """-> (render masks [S,H,W] u8, warp masks [Wn,H,W] u8, counts len [Wn,S] int32) of the latest run of a covered level, as
        numpy (host copies)."""
        h, w = self.ctx.height, self.ctx.width
        r = np.empty((self.S, h, w), np.uint8)
        m = np.empty((self.Wn, h, w), np.uint8)
        n = np.empty((self.Wn, self.S), np.int32)
        self.ctx._check(self._lib.nmi_level_copy_coverage(self._h, r.ctypes.data, m.ctypes.data, n.ctypes.data_as(C.POINTER(C.c_int32))),
                        "nmi_level_copy_coverage")
        return r, m, n

    def set_depth_shade(self, shade):
        """Depth renders (nmi_level_set_depth_shade): with an NmiDepthShade every replay's renders are the depth renders of the
        level's map; None turns them back into the map's colour (refused on a level created without attributes)."""
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_depth_shade(self._h, _shade_ref(shade, allow_none=True)), "nmi_level_set_depth_shade")
        self._shade = shade

    def set_peaks(self, K, num=None, radius=None):
        """Ranked peaks (nmi_level_set_peaks): every replay also ranks the K best separated candidates of its rating table, in one
        more node after the search.  num, radius: six ints each (axis order of nmi_host.h; prod(num[:3]) = S, prod(num[3:]) = Wn).
        K = 0 turns it off."""
        num6 = None if num is None else (C.c_int32 * 6)(*[int(v) for v in num])
        rad6 = None if radius is None else (C.c_int32 * 6)(*[int(v) for v in radius])
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_peaks(self._h, int(K), num6, rad6), "nmi_level_set_peaks")
        self._peaks_K = int(K)

    def copy_peaks(self):
        """-> (keys uint64 [K] numpy in rank order, zeros after the peaks; count) of the latest run of a level with peaks."""
        keys, n = np.zeros(PEAKS_MAX_K, np.uint64), C.c_int32(0)
        self.ctx._check(self._lib.nmi_level_copy_peaks(self._h, keys.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)), "nmi_level_copy_peaks")
        return keys[:getattr(self, "_peaks_K", 0)], int(n.value)

    def set_refine(self, on=True):
        """Refined peaks (nmi_level_set_refine): every replay also refines the peaks of set_peaks, in one more node behind theirs.
        Needs set_peaks with K > 0; set_peaks(0) turns it off too."""
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_refine(self._h, 1 if on else 0), "nmi_level_set_refine")

    def copy_refined(self):
        """-> (records REFINED_PEAK [K] numpy, record k for peak k of copy_peaks; count) of the latest run of a level with refined
        peaks."""
        records, n = np.zeros(PEAKS_MAX_K, REFINED_PEAK), C.c_int32(0)
        self.ctx._check(self._lib.nmi_level_copy_refined(self._h, records.ctypes.data, C.byref(n)), "nmi_level_copy_refined")
        return records[:getattr(self, "_peaks_K", 0)], int(n.value)

    def set_distortion(self, K, dist):
        """Distorted lens (nmi_level_set_distortion): the level's frame, and a frame mask given to set_masks / set_coverage, are
        then the RAW camera frame; every replay undistorts them for K ([3,3] float64) and dist = (k1, k2, p1, p2, k3) before the
        warps.  dist=None or all zeros turns it off."""
        k, d, kp, dp = _lens(K, dist)
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_distortion(self._h, kp, dp), "nmi_level_set_distortion")

    def set_distortion_fisheye(self, K, K_raw, dist):
        """Fisheye lens (nmi_level_set_distortion_fisheye): set_distortion for the equidistant model, K the pinhole camera of the
        renders, K_raw the raw frame's (None: K), dist = (k1, k2, k3, k4).  One lens setting per level: the later of the two calls
        wins; dist=None turns it off (four zeros do not)."""
        keep, (kp, krp, dp) = _fisheye(K, K_raw, dist)
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_distortion_fisheye(self._h, kp, krp, dp), "nmi_level_set_distortion_fisheye")

    def set_frame_format(self, fmt, pitch=0):
        """Colour or pitched frame (nmi_level_set_frame_format): every replay reads the level's frame in place as H rows of `pitch`
        bytes (0: dense) in format fmt (FRAME_*) and converts it to grey on the device (undistorting it in the same node when
        set_distortion is on).  Frame masks stay dense [H,W].  (FRAME_GRAY, 0) or (FRAME_GRAY, W) turns it off."""
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_frame_format(self._h, int(fmt), int(pitch)), "nmi_level_set_frame_format")

    def set_tone_map(self, tm=None):
        """Tone map of a FRAME_GRAY16 frame (nmi_level_set_tone_map; ToneMap, None: SHIFT, 16 bits): PERCENTILE, EQUALIZE and CLAHE
        take their statistics from the frame at every replay.  Ignored under every other format."""
        self.ctx._check(self._lib.nmi_level_set_tone_map(self._h, _tone_ref(tm)), "nmi_level_set_tone_map")
        self._tone = tm

    def set_valid_range(self, lo=0, hi=65535):
        """Valid range of a deep frame (nmi_level_set_valid_range): a pixel is valid iff lo <= raw <= hi.  Invalid pixels stay out
        of the tone map's statistics at every replay, and a masked or covered level's frame mask becomes the validity mask ANDed
        with the frame_mask given to set_masks / set_coverage (None: validity alone).  The level's own setting: the context's
        set_valid_range does not reach it.  (0, 65535) turns it off; ignored under every format that is not deep."""
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_valid_range(self._h, int(lo), int(hi)), "nmi_level_set_valid_range")

    def set_frame_reduction(self, factor, fmt=FRAME_GRAY, pitch=0):
        """Full-size frame (nmi_level_set_frame_reduction): every replay reads the level's frame in place as factor * H rows of
        `pitch` bytes (0: dense), each factor * W pixels in format fmt (FRAME_*), and reduces it to the grey frame of the search
        size on the device (reduce_frame's arithmetic), before the undistortion when set_distortion is on.  Frame masks stay
        [H,W].  set_frame_format with a factor: the later of the two calls wins; (1, FRAME_GRAY, 0) turns both off."""
        self.ctx._order_after_torch()
        self.ctx._check(self._lib.nmi_level_set_frame_reduction(self._h, int(factor), int(fmt), int(pitch)), "nmi_level_set_frame_reduction")

    def close(self):
        if self._h and self._h.value:
            self._lib.nmi_level_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class NmiStream:
    """nmi_stream wrapper: double-buffered keyframe pipeline (H2D of render stacks beside the search)."""

    def __init__(self, ctx, max_S, max_Wn, depth=2):
        self.ctx = ctx
        self._lib = ctx._lib
        self._h = C.c_void_p()
        ctx._check(self._lib.nmi_stream_create(ctx._h, int(max_S), int(max_Wn), int(depth), C.byref(self._h)),
                   "nmi_stream_create")
        self._keep = {}

    def submit(self, render_stack_host, frame_host=None, homographies=None, block=None, comm=None):
        """render_stack_host / frame_host: pinned CPU uint8 torch tensors; homographies: float64 [Wn,3,3] (with a frame).
        block = (s_offset, S_total, w_offset, Wn_total): the stack and the homographies are this rank's block of a level
        sharded over ranks (nmi_stream_submit_block); comm: RCCL communicator whose ranks all-reduce the level's key."""
        rs = render_stack_host
        if rs.is_cuda or rs.dtype.__str__() != "torch.uint8" or not rs.is_contiguous():
            raise TypeError("render_stack_host must be a contiguous CPU uint8 tensor (pinned for overlap)")
        fp, mp, wn, m = None, None, 0, None
        if frame_host is not None:
            m = np.ascontiguousarray(homographies, np.float64).reshape(-1, 9)
            fp = self._frame_ptr(frame_host) if hasattr(self, "_frame_bytes") else frame_host.data_ptr()
            mp, wn = m.ctypes.data_as(C.POINTER(C.c_double)), m.shape[0]
        t = C.c_int64(-1)
        if block is None and comm is None:
            self.ctx._check(self._lib.nmi_stream_submit(self._h, rs.data_ptr(), rs.shape[0], fp, mp, wn, C.byref(t)),
                            "nmi_stream_submit")
        else:
            if block is None:
                # a communicator without a block: a blockless level cannot say how many warps a frame-less submission reuses
                raise ValueError("NmiStream.submit(comm=...) needs block=(s_offset, S_total, w_offset, Wn_total): the position of this "
                                 "rank's views and warps in the level the ranks all-reduce over")
            so, st, wo, wt = (int(v) for v in block)
            self.ctx._check(self._lib.nmi_stream_submit_block(self._h, rs.data_ptr() if rs.shape[0] else None, rs.shape[0], so, st, fp, mp,
                                                              wn, wo, wt, comm, C.byref(t)), "nmi_stream_submit_block")
        self._keep[t.value] = (rs, frame_host, m)  # keep host buffers alive until the ticket completes
        return int(t.value)

    def _host_u8(self, t, what, nbytes):
        if t.is_cuda or str(t.dtype) != "torch.uint8" or not t.is_contiguous() or t.numel() != nbytes:
            raise TypeError(f"{what} must be a contiguous CPU uint8 tensor of {nbytes} bytes (pinned for overlap)")
        return t.data_ptr() if nbytes else None

    def _submit_masked(self, kind, render_stack_host, bits_host, frame_host, frame_mask_host, homographies, block, comm):
        rs = render_stack_host
        if rs.is_cuda or str(rs.dtype) != "torch.uint8" or not rs.is_contiguous():
            raise TypeError("render_stack_host must be a contiguous CPU uint8 tensor (pinned for overlap)")
        S, npix = rs.shape[0], self.ctx.width * self.ctx.height
        bp = None
        if kind == "covered":
            if bits_host is None:
                raise ValueError("submit_covered needs the render masks' bits (NmiContext.pack_mask_bits / np.packbits little)")
            bp = self._host_u8(bits_host, "render_mask_bits_host", S * ((npix + 7) // 8))
        fp, fmp, mp, wn, m = None, None, None, 0, None
        if frame_host is not None:
            m = np.ascontiguousarray(homographies, np.float64).reshape(-1, 9)
            fp, mp, wn = self._frame_ptr(frame_host), m.ctypes.data_as(C.POINTER(C.c_double)), m.shape[0]
        if frame_mask_host is not None:
            if frame_host is None:
                raise ValueError("frame_mask_host goes with a frame_host")
            fmp = self._host_u8(frame_mask_host, "frame_mask_host", npix)
        t = C.c_int64(-1)
        rp = rs.data_ptr() if S else None
        if block is None and comm is None:
            if kind == "covered":
                rc = self._lib.nmi_stream_submit_covered(self._h, rp, bp, S, fp, fmp, mp, wn, C.byref(t))
            else:
                rc = self._lib.nmi_stream_submit_masked(self._h, rp, S, fp, fmp, mp, wn, C.byref(t))
        else:
            if block is None:
                raise ValueError(f"NmiStream.submit_{kind}(comm=...) needs block=(s_offset, S_total, w_offset, Wn_total)")
            so, st, wo, wt = (int(v) for v in block)
            if kind == "covered":
                rc = self._lib.nmi_stream_submit_covered_block(self._h, rp, bp, S, so, st, fp, fmp, mp, wn, wo, wt, comm, C.byref(t))
            else:
                rc = self._lib.nmi_stream_submit_masked_block(self._h, rp, S, so, st, fp, fmp, mp, wn, wo, wt, comm, C.byref(t))
        self.ctx._check(rc, f"nmi_stream_submit_{kind}")
        self._keep[t.value] = (rs, bits_host, frame_host, frame_mask_host, m)  # host buffers stay alive until the ticket completes
        return int(t.value)

    def submit_masked(self, render_stack_host, frame_host=None, frame_mask_host=None, homographies=None, block=None, comm=None):
        """submit with warp masks (nmi_stream_submit_masked[_block]): the ticket equals nmi_warp_stack_masked + search_grid_masked.
        frame_mask_host: optional pinned CPU uint8 [H,W], nonzero = usable, only with a frame.  Without a frame the warps and warp
        masks of the most recent (masked or covered) frame are reused.  block / comm as for submit."""
        return self._submit_masked("masked", render_stack_host, None, frame_host, frame_mask_host, homographies, block, comm)

    def submit_covered(self, render_stack_host, render_mask_bits_host, frame_host=None, frame_mask_host=None, homographies=None,
                       block=None, comm=None):
        """submit with masks on both sides (nmi_stream_submit_covered[_block]): the ticket equals search_grid_covered on the
        render masks the bits came from.  render_mask_bits_host: pinned CPU uint8 [S, ceil(H*W/8)] (NmiContext.pack_mask_bits,
        or np.packbits(masks.reshape(S, -1) != 0, axis=1, bitorder="little")), render layout.  The rest as for submit_masked."""
        return self._submit_masked("covered", render_stack_host, render_mask_bits_host, frame_host, frame_mask_host, homographies,
                                   block, comm)

    def counts(self, ticket, n):
        """len_w [n = Wn] of a masked ticket or len[w][s] [n = Wn * S, layout [Wn][S]] of a covered ticket that has been waited
        for -> numpy int32 [n]."""
        out = np.zeros(int(n), np.int32)
        self.ctx._check(self._lib.nmi_stream_copy_counts(self._h, int(ticket), out.ctypes.data_as(C.POINTER(C.c_int32)), int(n)),
                        "nmi_stream_copy_counts")
        return out

    def set_distortion(self, K, dist):
        """Distorted lens (nmi_stream_set_distortion): frames (and frame masks) of later submissions, of every kind, are RAW and
        undistorted on the device for K ([3,3] float64) and dist = (k1, k2, p1, p2, k3) before their warps.  dist=None or all
        zeros turns it off."""
        k, d, kp, dp = _lens(K, dist)
        self.ctx._check(self._lib.nmi_stream_set_distortion(self._h, kp, dp), "nmi_stream_set_distortion")

    def set_distortion_fisheye(self, K, K_raw, dist):
        """Fisheye lens (nmi_stream_set_distortion_fisheye): set_distortion for the equidistant model, K the pinhole camera of the
        renders, K_raw the raw frame's (None: K), dist = (k1, k2, k3, k4).  The later of the two calls wins; dist=None turns it off."""
        keep, (kp, krp, dp) = _fisheye(K, K_raw, dist)
        self.ctx._check(self._lib.nmi_stream_set_distortion_fisheye(self._h, kp, krp, dp), "nmi_stream_set_distortion_fisheye")

    def set_frame_format(self, fmt, pitch=0):
        """Colour or pitched host frames (nmi_stream_set_frame_format): frames of later submissions, of every kind, are H rows of
        `pitch` bytes (0: dense) in format fmt (FRAME_*), converted to grey on the device before their warps.  Frame masks stay
        dense [H,W].  (FRAME_GRAY, 0) or (FRAME_GRAY, W) turns it off."""
        self.ctx._check(self._lib.nmi_stream_set_frame_format(self._h, int(fmt), int(pitch)), "nmi_stream_set_frame_format")
        self._frame_bytes = _frame_bytes(fmt, pitch, self.ctx.width, self.ctx.height)

    def set_tone_map(self, tm=None):
        """Tone map of FRAME_GRAY16 host frames (nmi_stream_set_tone_map; ToneMap, None: SHIFT, 16 bits), for later submissions:
        PERCENTILE, EQUALIZE and CLAHE take their statistics from each submitted frame."""
        self.ctx._check(self._lib.nmi_stream_set_tone_map(self._h, _tone_ref(tm)), "nmi_stream_set_tone_map")
        self._tone = tm

    def set_valid_range(self, lo=0, hi=65535):
        """Valid range of deep host frames (nmi_stream_set_valid_range), for later submissions: a pixel is valid iff lo <= raw <=
        hi.  Invalid pixels stay out of the tone map's statistics, and a masked or covered ticket's frame mask is the validity
        mask ANDed with frame_mask_host (None: validity alone), made on the device.  (0, 65535) turns it off."""
        self.ctx._check(self._lib.nmi_stream_set_valid_range(self._h, int(lo), int(hi)), "nmi_stream_set_valid_range")

    def set_frame_reduction(self, factor, fmt=FRAME_GRAY, pitch=0):
        """Full-size host frames (nmi_stream_set_frame_reduction): frames of later submissions, of every kind, are factor * H rows
        of `pitch` bytes (0: dense), each factor * W pixels in format fmt (FRAME_*), reduced to the grey frame of the search size
        on the device before their warps.  Frame masks stay [H,W].  set_frame_format with a factor: the later call wins;
        (1, FRAME_GRAY, 0) turns both off."""
        self.ctx._check(self._lib.nmi_stream_set_frame_reduction(self._h, int(factor), int(fmt), int(pitch)), "nmi_stream_set_frame_reduction")
        self._frame_bytes = _frame_bytes(fmt, pitch, int(factor) * self.ctx.width, int(factor) * self.ctx.height)

    def _frame_ptr(self, frame_host):
        """A host frame's pointer, its size checked against the frame format (dense grey: exactly H x W bytes)."""
        need = getattr(self, "_frame_bytes", self.ctx.width * self.ctx.height)
        if need == self.ctx.width * self.ctx.height:
            return self._host_u8(frame_host, "frame_host", need)
        if frame_host.is_cuda or str(frame_host.dtype) != "torch.uint8" or not frame_host.is_contiguous() or frame_host.numel() < need:
            raise TypeError(f"frame_host must be a contiguous CPU uint8 tensor of at least {need} bytes (pinned for overlap)")
        return frame_host.data_ptr()

    def keep_ratings(self, on=True):
        self.ctx._check(self._lib.nmi_stream_keep_ratings(self._h, int(bool(on))), "nmi_stream_keep_ratings")

    def ratings(self, ticket, Wn, S):
        """Rating table [Wn, S] of a ticket that has been waited for (needs keep_ratings())."""
        t = np.empty((Wn, S), np.float32)
        self.ctx._check(self._lib.nmi_stream_copy_ratings(self._h, int(ticket), t.ctypes.data_as(C.POINTER(C.c_float)), t.size),
                        "nmi_stream_copy_ratings")
        return t

    def wait(self, ticket):
        idx, sc = C.c_int64(0), C.c_float(0)
        self.ctx._check(self._lib.nmi_stream_wait(self._h, int(ticket), C.byref(idx), C.byref(sc)), "nmi_stream_wait")
        self._keep.pop(ticket, None)
        return int(idx.value), np.float32(sc.value)

    def close(self):
        if self._h and self._h.value:
            self._lib.nmi_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def rccl_unique_id():
    buf = (C.c_uint8 * 128)()
    rc = load_library().nmi_rccl_unique_id(buf)
    if rc != NMI_OK:
        raise NmiError(rc, "nmi_rccl_unique_id")
    return bytes(buf)


def rccl_comm_destroy(comm):
    load_library().nmi_rccl_comm_destroy(comm)
