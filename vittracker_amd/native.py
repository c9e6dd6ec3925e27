"""ctypes binding of ``libvittrack_hip.so`` (C ABI declared in ``include/vittrack.h``).

PyTorch is plumbing here: it owns device memory and streams; every kernel launch goes through
the C ABI with raw device pointers.  There is NO fallback: if the library is missing or a call
fails, an exception is raised (``VtError``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
#: VITTRACK_LIB=<path> selects another build of the fp32 library (A/B tools: tools/ab_stages.py, tools/block_stamps.py)
LIB_PATH = os.environ.get("VITTRACK_LIB") or os.path.join(_HERE, "csrc", "libvittrack_hip.so")
#: the same sources built with every vit_48 contraction on f16 MFMA (BASELINE config 5; make -C csrc all)
LIB_PATH_F16 = os.path.join(_HERE, "csrc", "libvittrack_hip_f16.so")
PRECISIONS = ("f32", "f16")


class VtError(RuntimeError):
    pass


class VtConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("template_size", "search_size", "channels", "heads", "depth",
                                         "head_channels", "stride", "max_batch")]


class VtTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


class VtOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")]


_vp, _i32, _f3p, _outp = C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(VtOutputs)
#: the C ABI of include/vittrack.h: name -> (restype, argtypes).  lib() applies it to each library, so a symbol cannot be exported
#: without its argument types (ctypes passes an undeclared argument as a C int: a 64-bit device pointer would be truncated)
ABI = {
    "vt_last_error": (C.c_char_p, []),
    "vt_version": (C.c_char_p, []),
    "vt_create": (C.c_int, [C.POINTER(VtConfig), C.POINTER(_vp)]),
    "vt_create_vit": (C.c_int, [C.POINTER(VtConfig), C.POINTER(_vp)]),
    "vt_destroy": (None, [_vp]),
    "vt_load_weights": (C.c_int, [_vp, C.POINTER(VtTensor), _i32]),
    "vt_set_window": (C.c_int, [_vp, _vp]),
    "vt_forward": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _outp]),
    "vt_stem": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp]),
    "vt_blocks": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "vt_head": (C.c_int, [_vp, _vp, _i32, _vp, _outp]),
    "vt_cal_bbox": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "vt_graph_capture": (C.c_int, [_vp, _vp, _vp, _i32, _outp, C.POINTER(_vp)]),
    "vt_graph_capture_steps": (C.c_int, [_vp, _i32, C.POINTER(_vp), C.POINTER(_vp), _i32, _outp, C.POINTER(_vp)]),
    "vt_graph_launch": (C.c_int, [_vp, _vp]),
    "vt_graph_destroy": (None, [_vp]),
    "vt_query": (C.c_int, [_vp] + [C.POINTER(_i32)] * 4),
    "vt_selftest_mfma": (C.c_int, [_vp]),
    "vt_probe_clock": (C.c_int, [_i32, _i32] + [C.POINTER(C.c_double)] * 3),
    "vt_debug_stamps": (C.c_int, [_vp, _i32, _vp]),
    "vt_update_state": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vt_update_state_record": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vt_set_template": (C.c_int, [_vp, _vp, _i32, _vp]),
    "vt_set_template_slots": (C.c_int, [_vp, _vp, C.POINTER(_i32), _i32, _vp]),
    "vt_set_form_batch": (C.c_int, [_vp, _i32]),
    "vt_set_normalization": (C.c_int, [_vp, _f3p, _f3p]),
    "vt_set_open_loop": (C.c_int, [_vp, _i32]),
    "vt_forward_u8": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _outp]),
    "vt_stem_u8": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
    "vt_patch_u8_supported": (C.c_int, [_vp, _i32]),
    "vt_crop_form": (C.c_int, []),
    "vt_gemm_form": (C.c_int, [_vp, _i32]),
    "vt_set_candidate_elimination": (C.c_int, [_vp, _i32, C.POINTER(_i32), C.POINTER(C.c_double), _vp]),
    "vt_set_ce_form": (C.c_int, [_vp, _i32]),
    "vt_ce_result": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
}
# the three frame sources of the crops and of the step: a dense (B,H,W,3) batch (frames, H, W), a vt_frame table, a vt_image table
for _sfx, _src in (("", [_vp, _i32, _i32]), ("_frames", [_vp]), ("_images", [_vp])):
    ABI["vt_crop" + _sfx] = (C.c_int, [_vp] + _src + [_vp, C.c_double, _i32, _f3p, _f3p, _i32, _vp, _vp, _vp])
    ABI["vt_crop_u8" + _sfx] = (C.c_int, [_vp] + _src + [_vp, C.c_double, _i32, _i32, _vp, _vp, _vp])
    ABI["vt_track_step" + _sfx] = (C.c_int, [_vp] + _src + [_vp, C.c_double, _f3p, _f3p, _i32, _vp, _vp, _vp, _vp, _i32, _vp])
#: every symbol include/vittrack.h declares (tests check the library exports all of them)
SYMBOLS = list(ABI)

_lib = None          # the fp32 library (kept as a module attribute: __graft_entry__.build() resets it)
_libs = {}


def lib(precision: str = "f32"):
    """Load a library once.  Raises VtError (never falls back) when it has not been built."""
    global _lib
    if precision not in PRECISIONS:
        raise VtError(f"unknown precision {precision!r}: 'f32' (default) or 'f16'")
    if precision == "f32" and _lib is not None:
        return _lib
    if precision != "f32" and precision in _libs:
        return _libs[precision]
    path = LIB_PATH if precision == "f32" else LIB_PATH_F16
    if not os.path.exists(path):
        raise VtError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C vittracker_amd/csrc all` (there is no CPU fallback)")
    # PyTorch-ROCm ships its own copy of the HIP runtime.  It has to be loaded before this library pulls in the
    # system libamdhip64: in the opposite order torch.cuda.is_available() turns False for the rest of the process
    # (seen when a process created a Model before it had ever imported torch).
    import torch  # noqa: F401
    L = C.CDLL(path)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if precision == "f32":
        _lib = L
    else:
        _libs[precision] = L
    return L


def _check(rc: int, what: str, L=None):
    if rc != 0:
        raise VtError(f"{what} failed ({rc}): {(L or lib()).vt_last_error().decode()}")


def _ptr(t):
    """Device pointer of a contiguous fp32 CUDA(HIP) tensor, or None."""
    if t is None:
        return None
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise VtError("expected a contiguous float32 tensor on the GPU, got "
                      f"{type(t).__name__} {getattr(t, 'dtype', '')} {getattr(t, 'device', '')}")
    return C.c_void_p(t.data_ptr())


def _f3(v):
    """The three floats of a per-channel mean or std, as the C ABI takes them."""
    return (C.c_float * 3)(*[float(x) for x in v])


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


#: struct vt_frame (include/vittrack.h): {const uint8_t* data; int32_t H, W; int64_t pitch;}, 24 bytes
FRAME_DTYPE = np.dtype([("data", "<u8"), ("H", "<i4"), ("W", "<i4"), ("pitch", "<i8")])
assert FRAME_DTYPE.itemsize == 24
#: frames packed into one arena start at multiples of this many bytes (vt_frame wants 4; 256 keeps every frame on its own cache lines)
ARENA_ALIGN = 256


def pack_planes(sizes, start: int = 0, align: int = ARENA_ALIGN):
    """Byte offsets of items packed one after the other from `start`, every plane of every item at a multiple of `align`.  sizes: per
    item the byte counts of its planes.  Returns ([per item: [plane offsets]], end)."""
    out, o = [], int(start)
    for planes in sizes:
        offs = []
        for n in planes:
            o = -(-o // align) * align
            offs.append(o)
            o += int(n)
        out.append(offs)
    return out, o


def pack_offsets(shapes, start: int = 0, align: int = ARENA_ALIGN):
    """Byte offsets of HWC uint8 frames of the given (H, W) shapes packed one after the other from `start`, each at a multiple of
    `align`, rows at pitch 3 W.  Returns (offsets, end)."""
    offs, end = pack_planes([[int(H) * int(W) * 3] for H, W in shapes], start, align)
    return [o[0] for o in offs], end


class _DescriptorTable:
    """A (B,) table of the descriptors of one frame per sequence (include/vittrack.h).  `host` is the numpy view of the descriptors
    (pinned when the table was made for a device); `dev` is the (B * ITEM,) uint8 device tensor the kernels read (upload() copies host
    -> dev); `keep` holds what the descriptors point into.  Subclasses give DTYPE and ITEM, KIND (the suffix of their entry points:
    vt_crop_<KIND>), WHAT (their name in ptr()'s message), the host-side check of one descriptor, and `_put`, the entry of one frame
    object."""

    def __init__(self, B: int, device=None):
        import torch
        self.B = int(B)
        pin = device is not None and torch.cuda.is_available()
        self._host_t = torch.zeros(self.B * self.ITEM, dtype=torch.uint8, pin_memory=pin)
        self.host = self._host_t.numpy().view(self.DTYPE)
        self.dev = None if device is None else torch.zeros(self.B * self.ITEM, dtype=torch.uint8, device=device)
        self.keep = [None] * self.B          # tensors the descriptors point into (kept alive with the table)
        self._copied = None                  # event of the last upload from the pinned host copy: _write() waits for it

    def _write(self, i: int, desc: tuple, keep):
        if self._copied is not None:         # the queued upload has not necessarily read the host copy yet
            self._copied.synchronize()
            self._copied = None
        self.host[i] = desc
        self.keep[i] = keep

    @classmethod
    def of(cls, items, device="cuda", stream=None):
        """A table of a list of frame objects on the GPU or in pinned memory (what `_put` takes), uploaded."""
        t = cls(len(items), device)
        for i, f in enumerate(items):
            t._put(i, f)
        t.upload(stream)
        return t

    def upload(self, stream=None):
        import torch
        if self.dev is None:
            raise VtError(f"this {type(self).__name__} has no device copy")
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.dev.copy_(self._host_t, non_blocking=self._host_t.is_pinned())
            if self._host_t.is_pinned():
                self._copied = torch.cuda.Event()
                self._copied.record()
        return self.dev

    @classmethod
    def ptr(cls, table, B):
        """Device address of a (B,) table of this class: an instance (its device copy) or a uint8 tensor of B * ITEM bytes."""
        import torch
        t = table.dev if isinstance(table, cls) else table
        if not (isinstance(t, torch.Tensor) and (t.is_cuda or t.is_pinned()) and t.numel() * t.element_size() >= B * cls.ITEM
                and t.is_contiguous()):
            raise VtError(f"{cls.WHAT} with a device copy or a contiguous tensor of {B} x {cls.ITEM} bytes on the GPU")
        return C.c_void_p(t.data_ptr())


class FrameTable(_DescriptorTable):
    """The (B,) vt_frame descriptor table of vt_crop_frames / vt_track_step_frames (include/vittrack.h): one frame per sequence,
    each with its own address, H, W and row pitch.  Every entry is checked on the host before anything runs: HWC uint8 rows of 3 W
    contiguous bytes, pitch >= 3 W, a 4-byte-aligned address, and (buffers) the frame inside its buffer."""

    DTYPE = FRAME_DTYPE
    ITEM = FRAME_DTYPE.itemsize
    KIND, WHAT = "frames", "frame table must be a FrameTable"

    @staticmethod
    def check(ptr: int, H: int, W: int, pitch: int = 0, nbytes: int | None = None):
        """Validate one descriptor; returns the pitch actually used (0 -> 3 W).  nbytes: bytes available from ptr (a buffer)."""
        H, W, pitch = int(H), int(W), int(pitch)
        if H < 1 or W < 1:
            raise VtError(f"frame of {H}x{W} pixels: H and W must be >= 1")
        pitch = pitch or 3 * W
        if pitch < 3 * W:
            raise VtError(f"row pitch {pitch} is shorter than a row (3 W = {3 * W} bytes)")
        if not ptr or int(ptr) % 4:
            raise VtError(f"frame address {int(ptr or 0):#x} is not 4-byte aligned (vt_frame.data must be)")
        need = pitch * (H - 1) + 3 * W
        if need > 0xfffffff0:
            raise VtError(f"a frame of {need} bytes is beyond the 32-bit offsets of the crop kernels")
        if nbytes is not None and need > int(nbytes):
            raise VtError(f"a {H}x{W} frame at pitch {pitch} needs {need} bytes, its buffer has {int(nbytes)}")
        return pitch

    def set(self, i: int, ptr: int, H: int, W: int, pitch: int = 0, nbytes: int | None = None, keep=None):
        pitch = self.check(ptr, H, W, pitch, nbytes)
        self._write(i, (int(ptr), int(H), int(W), pitch), keep)

    def set_tensor(self, i: int, frame, device_only: bool = True):
        """Entry i from an (H, W, 3) uint8 tensor on the GPU or in pinned host memory: its rows may be strided (a crop of a larger
        image), its pixels may not."""
        import torch
        if not (isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3):
            raise VtError("a frame must be an (H, W, 3) uint8 tensor")
        if device_only and not (frame.is_cuda or frame.is_pinned()):
            raise VtError("a frame must be on the GPU or in pinned host memory (the kernels read it in place)")
        H, W = int(frame.shape[0]), int(frame.shape[1])
        if frame.stride(2) != 1 or (W > 1 and frame.stride(1) != 3) or (H > 1 and frame.stride(0) < 3 * W):
            raise VtError(f"frame strides {tuple(frame.stride())}: pixels must be 3 contiguous bytes, rows at least 3 W apart")
        self.set(i, frame.data_ptr(), H, W, frame.stride(0) if H > 1 else 3 * W, keep=frame)

    _put = set_tensor

    def shapes(self):
        return [(int(h), int(w)) for h, w in zip(self.host["H"], self.host["W"])]


# ---- pixel formats (vt_crop_images & co.) -----------------------------------------------------------------------------------
#: vt_image.format (include/vittrack.h)
PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA, PIX_NV12, PIX_NV21 = range(6)
PIX_NAMES = ("rgb", "bgr", "rgba", "bgra", "nv12", "nv21")
#: struct vt_image (include/vittrack.h): {const uint8_t *plane0, *plane1; int64_t pitch0, pitch1; int32_t H, W, format, reserved;}
IMAGE_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("pitch0", "<i8"), ("pitch1", "<i8"), ("H", "<i4"), ("W", "<i4"),
                        ("format", "<i4"), ("reserved", "<i4")])
assert IMAGE_DTYPE.itemsize == 48


#: the layouts added to bits 0-7 of vt_image.format (6 and 7 are never assigned) ...
PIX_I420, PIX_YV12, PIX_YUYV, PIX_UYVY, PIX_P010, PIX_GRAY8 = range(8, 14)
PIX_LAYOUT_NAMES = dict(enumerate(PIX_NAMES))
PIX_LAYOUT_NAMES.update({PIX_I420: "i420", PIX_YV12: "yv12", PIX_YUYV: "yuyv", PIX_UYVY: "uyvy", PIX_P010: "p010", PIX_GRAY8: "gray8"})
#: ... the planar layouts (14 and 15 are never assigned): three full-height planes of single bytes, no alignment rule ...
PIX_RGBP, PIX_BGRP, PIX_I444, PIX_I422 = range(16, 20)
PIX_LAYOUT_NAMES.update({PIX_RGBP: "rgbp", PIX_BGRP: "bgrp", PIX_I444: "i444", PIX_I422: "i422"})
#: ... the V-first planar and the two-plane 4:2:2 / 4:4:4 layouts in bytes, the two-plane ones in MSB-aligned 16-bit words (20 and 27-31
#: are never assigned) ...
PIX_YV16, PIX_YV24, PIX_NV16, PIX_NV24, PIX_P210, PIX_P410 = range(21, 27)
PIX_LAYOUT_NAMES.update({PIX_YV16: "yv16", PIX_YV24: "yv24", PIX_NV16: "nv16", PIX_NV24: "nv24", PIX_P210: "p210", PIX_P410: "p410"})
#: ... the planar layouts in LSB-aligned little-endian 16-bit words, 32 | sub << 2 | dep: sub 0 / 1 / 2 / 3 = 4:2:0 / 4:2:2 / 4:4:4 / luma
#: only, dep 0 / 1 / 2 = 10 / 12 / 16 bits (dep 3 and everything above 46 are never assigned) ...
WIDE_SUBS = ("420", "422", "444", "gray")
WIDE_DEPTHS = (10, 12, 16)


def pix_wide(sub: str, depth: int) -> int:
    """The layout code of a planar 16-bit layout: sub "420" | "422" | "444" | "gray", depth 10 | 12 | 16."""
    if sub not in WIDE_SUBS or depth not in WIDE_DEPTHS:
        raise VtError(f"a 16-bit planar layout is sub in {WIDE_SUBS} and depth in {WIDE_DEPTHS}, got {sub!r}, {depth!r}")
    return 32 | WIDE_SUBS.index(sub) << 2 | WIDE_DEPTHS.index(depth)


PIX_I010, PIX_I012, PIX_I016 = (pix_wide("420", d) for d in WIDE_DEPTHS)
PIX_I210, PIX_I212, PIX_I216 = (pix_wide("422", d) for d in WIDE_DEPTHS)
PIX_I410, PIX_I412, PIX_I416 = (pix_wide("444", d) for d in WIDE_DEPTHS)
PIX_GRAY10, PIX_GRAY12, PIX_GRAY16 = (pix_wide("gray", d) for d in WIDE_DEPTHS)
_WIDE16 = tuple(pix_wide(s, d) for s in WIDE_SUBS for d in WIDE_DEPTHS)
PIX_LAYOUT_NAMES.update({pix_wide(s, d): {"420": "i0", "422": "i2", "444": "i4", "gray": "gray"}[s] + str(d) for s in WIDE_SUBS for d in WIDE_DEPTHS})
#: ... its bits 8-11 (the matrix of a YUV layout) and 12-15 (its range); bits 16-31 must be 0
PIX_MATRICES = ("bt601", "bt709")
PIX_RANGES = ("limited", "full")
_YUV420 = (PIX_NV12, PIX_NV21, PIX_I420, PIX_YV12, PIX_P010, PIX_I010, PIX_I012, PIX_I016)
_YUV422 = (PIX_YUYV, PIX_UYVY)
_PLANAR = (PIX_RGBP, PIX_BGRP, PIX_I444, PIX_I422)
_PLANAR_YUV = (PIX_I444, PIX_I422)
_WIDE422 = (PIX_YV16, PIX_NV16, PIX_P210, PIX_I210, PIX_I212, PIX_I216)
_WIDE444 = (PIX_YV24, PIX_NV24, PIX_P410, PIX_I410, PIX_I412, PIX_I416)
_WIDE_GRAY = (PIX_GRAY10, PIX_GRAY12, PIX_GRAY16)
_WIDE = (PIX_YV16, PIX_YV24, PIX_NV16, PIX_NV24, PIX_P210, PIX_P410) + _WIDE16
_WIDE_PAIRS = (PIX_NV16, PIX_NV24, PIX_P210, PIX_P410)                            # plane 1 holds (U, V) pairs, H rows
_WIDE_WORDS = (PIX_P210, PIX_P410) + _WIDE16                                      # two bytes a sample
_WIDE_LSB = tuple(c for c in _WIDE16 if c & 3 != 2)                               # fetched as aligned 16-bit loads: even addresses and pitches


def pix_format(layout: int, matrix: str = "bt601", range: str = "limited") -> int:      # noqa: A002  (the keyword the constructors take)
    """The vt_image.format word of a layout and its colour tags."""
    if matrix not in PIX_MATRICES:
        raise VtError(f"matrix must be one of {PIX_MATRICES}, got {matrix!r}")
    if range not in PIX_RANGES:
        raise VtError(f"range must be one of {PIX_RANGES}, got {range!r}")
    return int(layout) | (PIX_MATRICES.index(matrix) << 8) | (PIX_RANGES.index(range) << 12)


def pix_fields(fmt: int):
    """(layout, matrix bits, range bits, bits 16-31) of a format word."""
    fmt = int(fmt) & 0xffffffff
    return fmt & 0xff, (fmt >> 8) & 0xf, (fmt >> 12) & 0xf, fmt >> 16


def pix_name(fmt: int) -> str:
    return PIX_LAYOUT_NAMES.get(int(fmt) & 0xff, f"format {int(fmt)}").upper()


def _row_bytes(fmt: int, W: int):
    """Bytes of one row of plane 0 and of plane 1 (0: no plane 1)."""
    lay = fmt & 0xff
    if lay in _WIDE:      # chroma samples a row: W (4:4:4) or W / 2; twice as many in a plane of pairs; bytes doubled in 16-bit words
        b = 2 if lay in _WIDE_WORDS else 1
        if lay in _WIDE_GRAY:
            return b * W, 0
        return b * W, b * (W if lay in _WIDE444 else W // 2) * (2 if lay in _WIDE_PAIRS else 1)
    if lay in (PIX_NV12, PIX_NV21):
        return W, W
    if lay == PIX_P010:
        return 2 * W, 2 * W
    if lay in (PIX_I420, PIX_YV12):
        return W, W // 2
    if lay in _YUV422:
        return 2 * W, 0
    if lay == PIX_GRAY8:
        return W, 0
    if lay in _PLANAR:
        return W, (W // 2 if lay == PIX_I422 else W)
    return (4 if lay in (PIX_RGBA, PIX_BGRA) else 3) * W, 0


def _plane1_rows(fmt: int, H: int) -> int:
    """Rows of plane 1: H / 2, or H for I420 / YV12 (its two chroma planes of H / 2 rows lie back to back at one pitch), or 2 H for
    the planar layouts (two planes of H rows back to back)."""
    lay = fmt & 0xff
    if lay in _WIDE:      # planes of pairs: H rows; three-plane layouts: both chroma planes, of H / 2 rows (4:2:0) or H rows each
        return H if lay in _WIDE_PAIRS else (H if lay in _YUV420 else 2 * H)
    return 2 * H if lay in _PLANAR else (H if lay in (PIX_I420, PIX_YV12) else H // 2)


def _chroma_rows(fmt: int, H: int) -> int:
    """Rows of ONE chroma plane (the trailing plane begins pitch1 times this many bytes after plane 1)."""
    return H // 2 if fmt & 0xff in _YUV420 else H


class Image:
    """One frame in a pixel format the tracker reads directly (vt_image, include/vittrack.h): RGB, BGR, RGBA, BGRA, GRAY8, NV12, NV21,
    P010 / P016, I420, YV12, YUYV (YUY2), UYVY, planar RGB / BGR (CHW tensors), I444 or I422.
    Planes are numpy arrays (host: BatchedVitTracker packs them into its pinned arena) or uint8 tensors on the GPU (read in place).
    Rows may be strided (a pitch wider than the row), pixels may not.  Build one with the constructors: Image.rgb(a), .bgr(a),
    .rgba(a), .bgra(a) for (H, W, 3 | 4) arrays, .gray(a) for (H, W), .nv12(y, uv) / .nv21(y, vu) for an (H, W) luma plane and an
    (H/2, W/2, 2) chroma plane (H, W even), .p010(y, uv) for the same shapes in 16-bit samples, .i420(y, u, v) / .yv12(y, v, u) /
    .i420_buffer(buf) for planar 4:2:0, .yuyv(a) / .uyvy(a) for (H, W, 2) packed 4:2:2.  Every YUV constructor takes
    matrix="bt601" | "bt709" and range="limited" | "full" (default: BT.601 limited).  Planar frames: .chw(t) for a (3, H, W) array or
    tensor (images_from_chw(batch) for a (B, 3, H, W) one), .rgb_planar(r, g, b) / .bgr_planar(b, g, r), .i444(y, u, v) / .i422(y, u, v)
    for three planes that lie back to back; they are read as single bytes and need no alignment.  The wide layouts: .yv16(y, v, u) /
    .yv24(y, v, u), .nv16(y, uv) / .nv24(y, uv) with (H, W/2, 2) / (H, W, 2) pairs, .p210(y, uv) / .p410(y, uv) for those in MSB-aligned
    16-bit samples, .yuv16(y, u, v, depth=10 | 12 | 16, sub="420" | "422" | "444") for ffmpeg's yuv4xxpNNle (.i010: yuv420p10le) and
    .gray16(a, depth=) for grayNNle; 16-bit planes are uint16 / int16 arrays or tensors, or their uint8 views."""

    __slots__ = ("format", "planes", "H", "W", "pitches")

    def __init__(self, fmt: int, planes, H: int, W: int, pitches):
        self.format, self.planes, self.H, self.W, self.pitches = int(fmt), tuple(planes), int(H), int(W), tuple(int(p) for p in pitches)

    @staticmethod
    def _strides(a):
        """(shape, byte strides, on the GPU) of a uint8 numpy array or tensor; anything else raises."""
        import torch
        if isinstance(a, torch.Tensor):
            if a.dtype != torch.uint8:
                raise VtError(f"image planes must be uint8, got {a.dtype}")
            if not (a.is_cuda or a.device.type == "cpu"):
                raise VtError(f"image planes must be numpy arrays or GPU tensors, got a tensor on {a.device}")
            return tuple(a.shape), tuple(int(v) for v in a.stride()), a.is_cuda
        if isinstance(a, np.ndarray):
            if a.dtype != np.uint8:
                raise VtError(f"image planes must be uint8, got {a.dtype}")
            return a.shape, a.strides, False
        raise VtError(f"image planes must be numpy arrays or GPU tensors, got {type(a).__name__}")

    @classmethod
    def _packed(cls, fmt, a, C_):
        shape, st, _ = cls._strides(a)
        name = pix_name(fmt)
        if len(shape) != 3 or shape[2] != C_ or shape[0] < 1 or shape[1] < 1:
            raise VtError(f"a {name} image must be (H, W, {C_}), got {tuple(shape)}")
        H, W = int(shape[0]), int(shape[1])
        if st[2] != 1 or (W > 1 and st[1] != C_) or (H > 1 and st[0] < C_ * W):
            raise VtError(f"{name} strides {tuple(st)}: pixels must be {C_} contiguous bytes, rows at least {C_} W apart")
        return cls(fmt, (a,), H, W, (st[0] if H > 1 else C_ * W,))

    @classmethod
    def rgb(cls, a):
        return cls._packed(PIX_RGB, a, 3)

    @classmethod
    def bgr(cls, a):
        """A BGR frame as OpenCV hands it out (cv.imread, cv.VideoCapture)."""
        return cls._packed(PIX_BGR, a, 3)

    @classmethod
    def rgba(cls, a):
        return cls._packed(PIX_RGBA, a, 4)

    @classmethod
    def bgra(cls, a):
        return cls._packed(PIX_BGRA, a, 4)

    @classmethod
    def gray(cls, a):
        """An 8-bit grey frame (thermal / IR cameras), (H, W): rgb = (Y, Y, Y), no conversion."""
        shape, st, _ = cls._strides(a)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise VtError(f"a GRAY8 image must be (H, W), got {tuple(shape)}")
        H, W = int(shape[0]), int(shape[1])
        if (W > 1 and st[1] != 1) or (H > 1 and st[0] < W):
            raise VtError(f"GRAY8 strides {tuple(st)}: pixels must be contiguous bytes, rows at least W apart")
        return cls(PIX_GRAY8, (a,), H, W, (st[0] if H > 1 else W,))

    @classmethod
    def _yuv(cls, fmt, y, c, spp=1):
        """Two-plane 4:2:0: luma (H, W * spp) bytes and chroma pairs (H/2, W/2, 2 * spp) bytes; spp: bytes per sample."""
        sy, ty, gy = cls._strides(y)
        sc, tc, gc = cls._strides(c)
        name = pix_name(fmt)
        if len(sy) != 2 or sy[1] % spp:
            raise VtError(f"an {name} luma plane must be (H, W) with H and W even, got {tuple(sy)}")
        sy = (sy[0], sy[1] // spp)
        if sy[0] < 2 or sy[1] < 2 or sy[0] % 2 or sy[1] % 2:
            raise VtError(f"an {name} luma plane must be (H, W) with H and W even, got {tuple(sy)}")
        H, W = int(sy[0]), int(sy[1])
        if tuple(sc) != (H // 2, W // 2, 2 * spp):
            raise VtError(f"an {name} chroma plane must be (H/2, W/2, 2) = {(H // 2, W // 2, 2)}, got {(sc[0], sc[1], sc[2] // spp) if len(sc) == 3 else tuple(sc)}")
        if gy != gc:
            raise VtError(f"the two planes of an {name} image must both be on the GPU or both on the host")
        if ty[1] != 1 or ty[0] < W * spp:
            raise VtError(f"{name} luma strides {tuple(ty)}: pixels must be contiguous bytes, rows at least {'2 ' if spp == 2 else ''}W apart")
        if tc[2] != 1 or (W > 2 and tc[1] != 2 * spp) or (H > 2 and tc[0] < W * spp):
            raise VtError(f"{name} chroma strides {tuple(tc)}: pairs must be contiguous bytes, rows at least {'2 ' if spp == 2 else ''}W apart")
        return cls(fmt, (y, c), H, W, (ty[0], tc[0] if H > 2 else W * spp))

    @classmethod
    def nv12(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A decoder's NV12 surface: luma (H, W) and interleaved (U, V) pairs (H/2, W/2, 2)."""
        return cls._yuv(pix_format(PIX_NV12, matrix, range), y, uv)

    @classmethod
    def nv21(cls, y, vu, matrix="bt601", range="limited"):      # noqa: A002
        """NV21: as NV12 with (V, U) pairs."""
        return cls._yuv(pix_format(PIX_NV21, matrix, range), y, vu)

    @staticmethod
    def _bytes16(a, what, name="P010"):
        """A 16-bit plane as bytes (last axis doubled): uint16 / int16 numpy arrays and tensors, or their uint8 views as they are."""
        import torch
        if isinstance(a, np.ndarray):
            if a.dtype == np.uint8:
                return a
            if a.dtype.kind not in "ui" or a.dtype.itemsize != 2 or a.dtype.byteorder == ">":
                raise VtError(f"{name} {what} must be little-endian 16-bit samples or their uint8 view, got {a.dtype}")
            if a.ndim == 0 or a.strides[-1] != 2:
                raise VtError(f"{name} {what} strides {a.strides}: samples must be contiguous")
            return a.view(np.uint8)      # the last axis doubled; rows keep their stride
        if isinstance(a, torch.Tensor):
            if a.dtype == torch.uint8:
                return a
            if a.dtype not in (torch.int16, torch.uint16) or (a.dim() and a.shape[-1] > 1 and a.stride(-1) != 1):
                raise VtError(f"{name} {what} must be contiguous 16-bit samples or their uint8 view, got {a.dtype}")
            return a.view(torch.uint8)
        raise VtError(f"image planes must be numpy arrays or GPU tensors, got {type(a).__name__}")

    @classmethod
    def p010(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A 10-bit decoder's P010 surface (a P016 one is read the same way): NV12's layout in little-endian 16-bit samples -- luma
        (H, W) and (U, V) pairs (H/2, W/2, 2) as uint16 / int16 arrays or tensors, or their uint8 views (H, 2 W) and (H/2, W/2, 4).
        The 8-bit sample is the high byte of each word."""
        yb, cb = cls._bytes16(y, "luma"), cls._bytes16(uv, "chroma")
        return cls._yuv(pix_format(PIX_P010, matrix, range), yb, cb, spp=2)

    @classmethod
    def _planar(cls, fmt, y, c1, c2):
        sy, ty, gy = cls._strides(y)
        name = pix_name(fmt)
        if len(sy) != 2 or sy[0] < 2 or sy[1] < 2 or sy[0] % 2 or sy[1] % 2:
            raise VtError(f"an {name} luma plane must be (H, W) with H and W even, got {tuple(sy)}")
        H, W = int(sy[0]), int(sy[1])
        if ty[1] != 1 or ty[0] < W:
            raise VtError(f"{name} luma strides {tuple(ty)}: pixels must be contiguous bytes, rows at least W apart")
        pitch1 = None
        for c in (c1, c2):
            sc, tc, gc = cls._strides(c)
            if tuple(sc) != (H // 2, W // 2):
                raise VtError(f"an {name} chroma plane must be (H/2, W/2) = {(H // 2, W // 2)}, got {tuple(sc)}")
            if gc != gy:
                raise VtError(f"the planes of an {name} image must all be on the GPU or all on the host")
            if (W > 2 and tc[1] != 1) or (H > 2 and tc[0] < W // 2):
                raise VtError(f"{name} chroma strides {tuple(tc)}: pixels must be contiguous bytes, rows at least W/2 apart")
            q = tc[0] if H > 2 else None
            if pitch1 is not None and q is not None and q != pitch1:
                raise VtError(f"the two chroma planes of an {name} image must have one row pitch, got {pitch1} and {q}")
            pitch1 = q if q is not None else pitch1
        pitch1 = pitch1 if pitch1 is not None else W // 2
        if gy and int(c2.data_ptr()) != int(c1.data_ptr()) + pitch1 * (H // 2):
            # the descriptor has one plane-1 pointer: the second chroma plane is found pitch1 * H/2 bytes after the first
            raise VtError(f"the chroma planes of a device {name} image are not contiguous: the second must begin pitch1 * H/2 = "
                          f"{pitch1 * (H // 2)} bytes after the first (one buffer, as Image.i420_buffer takes); copy them into one")
        return cls(fmt, (y, c1, c2), H, W, (ty[0], pitch1))

    @classmethod
    def i420(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:2:0 as software decoders produce it (ffmpeg's yuv420p): luma (H, W), U and V (H/2, W/2) each.  On the GPU the V
        plane must begin pitch1 * H/2 bytes after the U plane; host planes are packed that way into the arena."""
        return cls._planar(pix_format(PIX_I420, matrix, range), y, u, v)

    @classmethod
    def yv12(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV12: I420 with the V plane first."""
        return cls._planar(pix_format(PIX_YV12, matrix, range), y, v, u)

    @classmethod
    def i420_buffer(cls, buf, matrix="bt601", range="limited"):      # noqa: A002
        """One contiguous I420 buffer as OpenCV (COLOR_YUV2RGB_I420) and av_image_copy_to_buffer lay it out: a (3H/2, W) array of tight
        rows -- H rows of luma, then the U plane, then the V plane (H/2 rows of W/2 bytes each)."""
        shape, st, _ = cls._strides(buf)
        if len(shape) != 2 or shape[0] < 3 or shape[0] % 3 or shape[1] < 2 or shape[1] % 2:
            raise VtError(f"an I420 buffer must be (3H/2, W) with H and W even, got {tuple(shape)}")
        H, W = 2 * int(shape[0]) // 3, int(shape[1])
        if st[1] != 1 or st[0] != W:
            raise VtError(f"I420 buffer strides {tuple(st)}: rows must be tight (W bytes apart), the chroma planes follow the luma plane")
        c = buf[H:].reshape(H, W // 2)      # both chroma planes, H / 2 rows each: a view
        return cls(pix_format(PIX_I420, matrix, range), (buf[:H], c), H, W, (W, W // 2))

    @classmethod
    def _packed422(cls, fmt, a):
        shape, st, _ = cls._strides(a)
        name = pix_name(fmt)
        if len(shape) != 3 or shape[2] != 2 or shape[0] < 1 or shape[1] < 2 or shape[1] % 2:
            raise VtError(f"a {name} image must be (H, W, 2) with W even, got {tuple(shape)}")
        H, W = int(shape[0]), int(shape[1])
        if st[2] != 1 or st[1] != 2 or (H > 1 and st[0] < 2 * W):
            raise VtError(f"{name} strides {tuple(st)}: pixels must be 2 contiguous bytes, rows at least 2 W apart")
        return cls(fmt, (a,), H, W, (st[0] if H > 1 else 2 * W,))

    @classmethod
    def yuyv(cls, a, matrix="bt601", range="limited"):      # noqa: A002
        """Packed 4:2:2 as capture cards and webcams produce it (YUY2): (H, W, 2), each 4 bytes Y0 U Y1 V."""
        return cls._packed422(pix_format(PIX_YUYV, matrix, range), a)

    @classmethod
    def uyvy(cls, a, matrix="bt601", range="limited"):      # noqa: A002
        """UYVY: each 4 bytes U Y0 V Y1."""
        return cls._packed422(pix_format(PIX_UYVY, matrix, range), a)

    @staticmethod
    def _address(a) -> int:
        return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a.__array_interface__["data"][0])

    @classmethod
    def _planar3(cls, fmt, p0, p1, p2, spp=1):
        """Three planes of single bytes (RGBP / BGRP, I444, I422 / YV16: chroma planes of W / 2 columns) or, spp = 2, of 16-bit samples
        given as bytes (the planar 16-bit layouts; 4:2:0: chroma planes of H / 2 rows).  The descriptor has two plane pointers and two
        pitches: the trailing planes must share one row pitch and the third must begin pitch1 * (its rows) bytes after the second.
        Planes that lie otherwise raise; nothing is copied here."""
        lay = fmt & 0xff
        name = pix_name(fmt)
        half = lay in (PIX_I422,) + _WIDE422 + _YUV420      # chroma planes of W / 2 columns
        s0, t0, g0 = cls._strides(p0)
        if len(s0) == 2 and s0[1] % spp == 0:
            s0 = (s0[0], s0[1] // spp)
        if len(s0) != 2 or s0[0] < 1 or s0[1] < 1 or (half and s0[1] % 2) or (lay in _YUV420 and s0[0] % 2):
            raise VtError(f"the first plane of an {name} image must be (H, W){' with W even' if half else ''}"
                          f"{' and H even' if lay in _YUV420 else ''}, got {tuple(s0)}")
        H, W = int(s0[0]), int(s0[1])
        if (W * spp > 1 and t0[1] != 1) or (H > 1 and t0[0] < W * spp):
            raise VtError(f"{name} plane 0 strides {tuple(t0)}: pixels must be contiguous bytes, rows at least {'2 ' if spp == 2 else ''}W apart")
        cw, ch = (W // 2 if half else W) * spp, _chroma_rows(fmt, H)
        pitch1 = None
        for c in (p1, p2):
            sc, tc, gc = cls._strides(c)
            if tuple(sc) != (ch, cw):
                raise VtError(f"the trailing planes of an {name} image must be {(ch, cw // spp)}, got "
                              f"{(sc[0], sc[1] // spp) if len(sc) == 2 else tuple(sc)}")
            if gc != g0:
                raise VtError(f"the planes of an {name} image must all be on the GPU or all on the host")
            if (cw > 1 and tc[1] != 1) or (ch > 1 and tc[0] < cw):
                raise VtError(f"{name} plane strides {tuple(tc)}: pixels must be contiguous bytes, rows at least {cw} apart")
            q = tc[0] if ch > 1 else None
            if pitch1 is not None and q is not None and q != pitch1:
                raise VtError(f"the two trailing planes of an {name} image must have one row pitch, got {pitch1} and {q}")
            pitch1 = q if q is not None else pitch1
        gap = cls._address(p2) - cls._address(p1)
        if pitch1 is None:      # one row: the pitch is what lies between the two planes
            pitch1 = gap
        if gap != pitch1 * ch or pitch1 < cw:
            raise VtError(f"the trailing planes of an {name} image are not back to back: the third must begin pitch1 * {'H/2' if ch != H else 'H'} = "
                          f"{pitch1 * ch} bytes after the second, it begins {gap} bytes after it (the descriptor has one pointer and "
                          f"one pitch for both); put them into one buffer, e.g. a (3, H, W) array for Image.chw")
        return cls(fmt, (p0, p1, p2), H, W, (t0[0] if H > 1 else W * spp, pitch1))

    @classmethod
    def _pairs(cls, fmt, y, c, spp=1):
        """Two planes at full height: luma (H, W) and (U, V) pairs (H, W/2, 2) (4:2:2) or (H, W, 2) (4:4:4), in bytes or, spp = 2, in
        16-bit samples given as bytes."""
        lay = fmt & 0xff
        name = pix_name(fmt)
        half = lay in _WIDE422
        sy, ty, gy = cls._strides(y)
        sc, tc, gc = cls._strides(c)
        if len(sy) == 2 and sy[1] % spp == 0:
            sy = (sy[0], sy[1] // spp)
        if len(sy) != 2 or sy[0] < 1 or sy[1] < 1 or (half and sy[1] % 2):
            raise VtError(f"an {name} luma plane must be (H, W){' with W even' if half else ''}, got {tuple(sy)}")
        H, W = int(sy[0]), int(sy[1])
        cw = W // 2 if half else W
        if tuple(sc) != (H, cw, 2 * spp):
            raise VtError(f"an {name} chroma plane must be {(H, cw, 2)}, got {(sc[0], sc[1], sc[2] // spp) if len(sc) == 3 else tuple(sc)}")
        if gy != gc:
            raise VtError(f"the two planes of an {name} image must both be on the GPU or both on the host")
        if (W * spp > 1 and ty[1] != 1) or (H > 1 and ty[0] < W * spp):
            raise VtError(f"{name} luma strides {tuple(ty)}: pixels must be contiguous bytes, rows at least {'2 ' if spp == 2 else ''}W apart")
        if tc[2] != 1 or (cw > 1 and tc[1] != 2 * spp) or (H > 1 and tc[0] < 2 * spp * cw):
            raise VtError(f"{name} chroma strides {tuple(tc)}: pairs must be contiguous bytes, rows at least {2 * spp * cw} bytes apart")
        return cls(fmt, (y, c), H, W, (ty[0] if H > 1 else W * spp, tc[0] if H > 1 else 2 * spp * cw))

    @classmethod
    def yv16(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV16: I422 with the V plane first; U begins pitch1 * H bytes after V."""
        return cls._planar3(pix_format(PIX_YV16, matrix, range), y, v, u)

    @classmethod
    def yv24(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV24: I444 with the V plane first."""
        return cls._planar3(pix_format(PIX_YV24, matrix, range), y, v, u)

    @classmethod
    def nv16(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """Two-plane 4:2:2 as capture cards produce it: luma (H, W) and (U, V) pairs (H, W/2, 2); W even."""
        return cls._pairs(pix_format(PIX_NV16, matrix, range), y, uv)

    @classmethod
    def nv24(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """Two-plane 4:4:4: luma (H, W) and (U, V) pairs (H, W, 2)."""
        return cls._pairs(pix_format(PIX_NV24, matrix, range), y, uv)

    @classmethod
    def p210(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A hardware decoder's P210 surface (a P216 one is read the same way): NV16 in little-endian 16-bit samples, as uint16 /
        int16 arrays or tensors (H, W) and (H, W/2, 2), or their uint8 views.  The 8-bit sample is the high byte of each word."""
        return cls._pairs(pix_format(PIX_P210, matrix, range), cls._bytes16(y, "luma", "P210"), cls._bytes16(uv, "chroma", "P210"), spp=2)

    @classmethod
    def p410(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """P410 / P416: NV24 in little-endian 16-bit samples, (H, W) and (H, W, 2); the high byte of each word."""
        return cls._pairs(pix_format(PIX_P410, matrix, range), cls._bytes16(y, "luma", "P410"), cls._bytes16(uv, "chroma", "P410"), spp=2)

    @classmethod
    def yuv16(cls, y, u, v, depth=10, sub="420", matrix="bt601", range="limited"):      # noqa: A002
        """Planar YUV in LSB-aligned little-endian 16-bit samples (ffmpeg's yuv420p10le ... yuv444p16le): depth 10 | 12 | 16, sub "420"
        | "422" | "444"; luma (H, W), U and V (H/2, W/2), (H, W/2) or (H, W) as uint16 / int16 arrays or tensors, or their uint8 views
        (last axis doubled).  The 8-bit sample is min(word >> (depth - 8), 255).  V must begin pitch1 * (chroma rows) bytes after U;
        10- and 12-bit planes must lie at even addresses and even pitches (they are fetched as 16-bit words)."""
        if sub not in WIDE_SUBS[:3]:
            raise VtError(f"sub must be one of {WIDE_SUBS[:3]}, got {sub!r}")
        lay = pix_wide(sub, depth)
        name = pix_name(lay)
        return cls._planar3(pix_format(lay, matrix, range), cls._bytes16(y, "luma", name), cls._bytes16(u, "chroma", name),
                            cls._bytes16(v, "chroma", name), spp=2)

    @classmethod
    def i010(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """yuv420p10le, what software HEVC Main10 / AV1 10-bit decoders produce: Image.yuv16(y, u, v, depth=10, sub="420")."""
        return cls.yuv16(y, u, v, 10, "420", matrix, range)

    @classmethod
    def gray16(cls, a, depth=16):
        """A grey frame in LSB-aligned little-endian 16-bit samples (gray10le / gray12le / gray16le; thermal and scientific cameras),
        (H, W) uint16 / int16 or its uint8 view (H, 2 W): rgb = (s, s, s) with s = min(word >> (depth - 8), 255)."""
        lay = pix_wide("gray", depth)
        name = pix_name(lay)
        ab = cls._bytes16(a, "plane", name)
        shape, st, _ = cls._strides(ab)
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 2 or shape[1] % 2:
            raise VtError(f"a {name} image must be (H, W) 16-bit samples, got {tuple(getattr(a, 'shape', ()))}")
        H, W = int(shape[0]), int(shape[1]) // 2
        if st[1] != 1 or (H > 1 and st[0] < 2 * W):
            raise VtError(f"{name} strides {tuple(st)}: samples must be contiguous, rows at least 2 W bytes apart")
        return cls(lay, (ab,), H, W, (st[0] if H > 1 else 2 * W,))

    @classmethod
    def rgb_planar(cls, r, g, b):
        """Planar RGB: three (H, W) planes.  G and B must share one row pitch with B beginning pitch * H bytes after G (the planes of a
        (3, H, W) array lie so); R may be anywhere."""
        return cls._planar3(PIX_RGBP, r, g, b)

    @classmethod
    def bgr_planar(cls, b, g, r):
        """Planar BGR: as rgb_planar with the B plane first."""
        return cls._planar3(PIX_BGRP, b, g, r)

    @classmethod
    def i444(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:4:4 (ffmpeg's yuv444p; screen capture): luma, U and V, (H, W) each; V begins pitch1 * H bytes after U."""
        return cls._planar3(pix_format(PIX_I444, matrix, range), y, u, v)

    @classmethod
    def i422(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:2:2 (yuv422p): luma (H, W), U and V (H, W/2) each, W even; V begins pitch1 * H bytes after U."""
        return cls._planar3(pix_format(PIX_I422, matrix, range), y, u, v)

    @classmethod
    def chw(cls, t, order="rgb"):
        """A (3, H, W) uint8 frame as torchvision.io.read_image / decode_jpeg and CHW dataloaders hand it out -- a numpy array, a CPU
        tensor or a CUDA tensor (read in place) --, with no copy.  The last dimension must be dense; row pitch and plane spacing come
        from the strides (a contiguous frame, a frame of a contiguous (B, 3, H, W) batch, rows padded to a pitch with planes pitch * H
        apart).  A view whose strides are those of a permuted (H, W, 3) array is taken as the packed frame it is.  order: "rgb" or
        "bgr", the meaning of the three planes."""
        if order not in ("rgb", "bgr"):
            raise VtError(f"order must be 'rgb' or 'bgr', got {order!r}")
        shape, st, _ = cls._strides(t)
        if len(shape) != 3 or shape[0] != 3 or shape[1] < 1 or shape[2] < 1:
            raise VtError(f"a CHW image must be (3, H, W), got {tuple(shape)}")
        if st[0] == 1 and st[2] == 3:      # a permuted HWC array: packed pixels
            hwc = t.permute(1, 2, 0) if hasattr(t, "permute") else t.transpose(1, 2, 0)
            return cls._packed(PIX_RGB if order == "rgb" else PIX_BGR, hwc, 3)
        if shape[2] > 1 and st[2] != 1:
            raise VtError(f"CHW strides {tuple(st)}: the last dimension must be dense (or the view a permuted (H, W, 3) array)")
        return cls._planar3(PIX_RGBP if order == "rgb" else PIX_BGRP, t[0], t[1], t[2])

    @property
    def is_cuda(self) -> bool:
        import torch
        return isinstance(self.planes[0], torch.Tensor) and self.planes[0].is_cuda

    @property
    def shape(self):
        """(H, W, 3): the shape of the RGB image it denotes."""
        return (self.H, self.W, 3)

    def plane_rows(self):
        """Per plane of the descriptor: (rows, row bytes).  I420 / YV12: plane 1 is both chroma planes back to back, H rows of W / 2;
        the planar layouts: both trailing planes, 2 H rows."""
        r0, r1 = _row_bytes(self.format, self.W)
        return [(self.H, r0)] + ([(_plane1_rows(self.format, self.H), r1)] if r1 else [])

    def host_planes(self):
        """The host planes as plane_rows() counts them: three separate planes (I420 / YV12, the planar layouts) give plane 0 and the two
        trailing planes stacked."""
        pl = [p.numpy() if hasattr(p, "numpy") else np.asarray(p) for p in self.planes]
        if len(pl) == 3:
            return [pl[0], np.concatenate([pl[1], pl[2]], axis=0)]
        return pl

    def descriptor(self, ptrs=None, pitches=None):
        """The vt_image tuple of this image: at its planes' own addresses (device images), or at `ptrs` with `pitches`."""
        if ptrs is None:
            ptrs = [int(p.data_ptr()) for p in self.planes]
            pitches = self.pitches
        return (int(ptrs[0]), int(ptrs[1]) if len(ptrs) > 1 else 0, int(pitches[0]), int(pitches[1]) if len(pitches) > 1 else 0,
                self.H, self.W, self.format, 0)


def images_from_chw(batch, order="rgb"):
    """A (B, 3, H, W) uint8 batch (numpy array, CPU or CUDA tensor) as a list of B Images that share its memory: Image.chw of every
    frame, no copy.  What BatchedVitTracker.initialize / track take in place of batch.permute(0, 2, 3, 1).contiguous()."""
    shape = tuple(getattr(batch, "shape", ()))
    if len(shape) != 4 or shape[1] != 3:
        raise VtError(f"a CHW batch must be (B, 3, H, W), got {shape}")
    return [Image.chw(batch[b], order) for b in range(shape[0])]


def pack_image_offsets(images, start: int = 0, align: int = ARENA_ALIGN):
    """Byte offsets of the planes of host Images packed one after the other from `start` at tight pitches, every plane at a
    multiple of `align`.  Returns ([per image: [plane offsets]], end)."""
    return pack_planes([[rows * rb for rows, rb in im.plane_rows()] for im in images], start, align)


class ImageTable(_DescriptorTable):
    """The (B,) vt_image descriptor table of vt_crop_images / vt_track_step_images (include/vittrack.h): one frame per sequence in
    its own pixel format, size and plane pitches."""

    DTYPE = IMAGE_DTYPE
    ITEM = IMAGE_DTYPE.itemsize
    KIND, WHAT = "images", "image table must be an ImageTable"

    @staticmethod
    def check(fmt: int, ptr0: int, ptr1: int, H: int, W: int, pitch0: int = 0, pitch1: int = 0, reserved: int = 0,
              nbytes0: int | None = None, nbytes1: int | None = None):
        """The device's rules for an unusable descriptor, on the host: raises VtError where the kernels would poison the sequence.
        Returns the pitches actually used (0 -> the row's bytes).  nbytes0 / nbytes1: bytes available from each plane (buffers)."""
        fmt, H, W, pitch0, pitch1 = int(fmt), int(H), int(W), int(pitch0), int(pitch1)
        lay, mat, rng, high = pix_fields(fmt)
        if lay not in PIX_LAYOUT_NAMES:
            raise VtError(f"unknown pixel format {fmt}")
        if high or mat >= len(PIX_MATRICES) or rng >= len(PIX_RANGES):
            raise VtError(f"unknown pixel format {fmt:#x}: matrix {mat}, range {rng}, bits 16-31 {high:#x}")
        if (mat or rng) and (lay not in _YUV420 + _YUV422 + _PLANAR_YUV + _WIDE or lay in _WIDE_GRAY):
            raise VtError(f"a {pix_name(fmt)} image takes no matrix or range bits, got format {fmt:#x}")
        if int(reserved) != 0:
            raise VtError("vt_image.reserved must be 0")
        if H < 1 or W < 1 or H > 0x10000000 or W > 0x10000000:
            raise VtError(f"image of {H}x{W} pixels: H and W must be >= 1")
        if lay in _YUV420 and (H % 2 or W % 2):
            raise VtError(f"an {pix_name(fmt)} image must have even H and W, got {H}x{W}")
        if lay in _YUV422 + (PIX_I422,) + _WIDE422 and W % 2:
            raise VtError(f"a {pix_name(fmt)} image must have even W, got {H}x{W}")
        r0, r1 = _row_bytes(fmt, W)
        planes = [(ptr0, pitch0, H, r0, nbytes0)] + ([(ptr1, pitch1, _plane1_rows(fmt, H), r1, nbytes1)] if r1 else [])
        used = []
        for k, (ptr, pitch, rows, rb, nb) in enumerate(planes):
            pitch = pitch or rb
            if pitch < rb:
                raise VtError(f"plane {k}: row pitch {pitch} is shorter than a row ({rb} bytes)")
            if not ptr or (int(ptr) % 4 and lay not in _PLANAR + _WIDE):      # the planar and wide layouts are read as single bytes: any address
                raise VtError(f"plane {k}: address {int(ptr or 0):#x} is null or not 4-byte aligned")
            if lay in _WIDE_LSB and (int(ptr) % 2 or pitch % 2):      # ... but for 10- and 12-bit words, fetched as aligned 16-bit loads
                raise VtError(f"plane {k}: address {int(ptr):#x} or row pitch {pitch} is odd; the 16-bit samples of a {pix_name(fmt)} image "
                              f"must be 2-byte aligned")
            need = pitch * (rows - 1) + rb
            if pitch > 0xfffffff0 or need > 0xfffffff0:
                raise VtError(f"plane {k}: {need} bytes are beyond the 32-bit offsets of the crop kernels")
            if nb is not None and need > int(nb):
                raise VtError(f"plane {k}: needs {need} bytes, its buffer has {int(nb)}")
            used.append(pitch)
        return used[0], (used[1] if len(used) > 1 else int(pitch1))

    def set(self, i: int, desc, keep=None, check: bool = True):
        """Entry i from a vt_image tuple (plane0, plane1, pitch0, pitch1, H, W, format, reserved); check=False writes it as it is."""
        p0, p1, q0, q1, H, W, fmt, res = (int(v) for v in desc)
        if check:
            q0, q1 = self.check(fmt, p0, p1, H, W, q0, q1, res)
        self._write(i, (p0, p1, q0, q1, H, W, fmt, res), keep)

    def set_image(self, i: int, image: Image):
        """Entry i from an Image whose planes are on the GPU (read in place)."""
        if not isinstance(image, Image) or not image.is_cuda:
            raise VtError("ImageTable.set_image wants an Image whose planes are on the GPU")
        self.set(i, image.descriptor(), keep=image)

    _put = set_image


# the device-pointer check under its two earlier names (tests/test_gpu_patch_u8.py calls the C ABI with them)
_table_ptr, _image_table_ptr = FrameTable.ptr, ImageTable.ptr


def ce_keep_counts(len_x: int, keep_ratio):
    """Search tokens kept after each candidate-elimination stage: math.ceil(keep_ratio * lens_s) of lib/models/layers/attn_blocks.py:39
    applied stage after stage (0.7, 0.7, 0.7: 180 / 126 / 89 of 256, 404 / 283 / 199 of 576).  The library computes the same."""
    import math
    out, n = [], int(len_x)
    for r in keep_ratio:
        if not 0.0 < float(r) <= 1.0:
            raise VtError(f"keep ratio {r} outside (0, 1]")
        n = min(n, max(1, math.ceil(float(r) * n)))
        out.append(n)
    return out


#: the bits of Model.gemm_form (include/vittrack.h VT_GEMM_*): the GEMM kinds that run on the narrow tile
GEMM_PATCH, GEMM_QK, GEMM_PROJ, GEMM_FC1, GEMM_FC2, GEMM_HEAD = 1, 2, 4, 8, 16, 32

#: the forms candidate elimination runs in (include/vittrack.h VT_CE_MASKED / VT_CE_COMPACT)
CE_FORMS = {"masked": 0, "compact": 1}


def ce_form_name(form=None) -> str:
    """The form's name: `form`, or without one the environment variable VB_CE_FORM, or "masked"."""
    if form is None:
        form = os.environ.get("VB_CE_FORM") or "masked"
    if form not in CE_FORMS:
        raise VtError(f"candidate elimination form {form!r}: one of {sorted(CE_FORMS)}")
    return form


def ce_compact_lengths(len_z: int, len_x: int, keep_ratio):
    """Rows of a frame behind each stage in the compact form: template rows + kept search tokens, rounded up to 16
    (0.7, 0.7, 0.7: 256 / 192 / 160 at 64 + 256 tokens, 560 / 432 / 352 at 144 + 576)."""
    return [(int(len_z) + k + 15) // 16 * 16 for k in ce_keep_counts(len_x, keep_ratio)]


def crop_form() -> int:
    """Which crop kernel form the current device runs: 1 = 8-byte unaligned windows (crop_fast_kernel / crop_kernel<false>), 2 = the
    byte-load fallback the device self test selects on any mismatch."""
    return int(lib().vt_crop_form())


def probe_clock(iters=20000, waves_per_simd=1):
    """(shader MHz under dense f32 MFMA, SIMD cycles per MFMA, wall us) -- development probe."""
    v = [C.c_double() for _ in range(3)]
    _check(lib().vt_probe_clock(iters, waves_per_simd, *[C.byref(x) for x in v]), "vt_probe_clock")
    return tuple(x.value for x in v)


def selftest_mfma():
    _check(lib().vt_selftest_mfma(_stream(None)), "vt_selftest_mfma")


class Outputs:
    """Torch-owned device buffers for one forward of batch B (the dict the reference returns)."""

    def __init__(self, B, F, device):
        import torch
        self.score_map = torch.empty(B, 1, F, F, device=device)
        self.size_map = torch.empty(B, 2, F, F, device=device)
        self.offset_map = torch.empty(B, 2, F, F, device=device)
        self.pred_boxes = torch.empty(B, 4, device=device)
        self.hann_boxes = torch.empty(B, 4, device=device)
        self.conf = torch.empty(B, device=device)

    def struct(self):
        return VtOutputs(*[C.c_void_p(getattr(self, n).data_ptr()) for n, _ in VtOutputs._fields_])


class Graph:
    """A captured step.  It holds its Model (the graph's kernels read the model's weight and workspace
    buffers) and the tensors it was captured on; when the model is closed or re-sized the graph is
    invalidated and ``launch`` raises instead of replaying kernels over freed memory."""

    def __init__(self, handle, keep, model=None):
        self._h = handle
        self._keep = keep   # tensors the captured kernels read / write
        self._model = model
        self._L = model._L if model is not None else lib()
        self._valid = True

    def launch(self, stream=None):
        if not self._valid:
            raise VtError("this graph was captured from a model that has since been closed or re-sized "
                          "(its weight / workspace buffers are gone): capture it again")
        _check(self._L.vt_graph_launch(self._h, _stream(stream)), "vt_graph_launch", self._L)

    def _invalidate(self):
        self._valid = False

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_L", None) is not None:
            try:
                self._L.vt_graph_destroy(self._h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self._h = None


class Model:
    """Owns one ``vt_model`` (weights + workspace on the current device)."""

    ce_form = "masked"      # the form set_candidate_elimination chose

    def __init__(self, template_size, search_size, channels=48, heads=1, depth=3, head_channels=32, stride=16,
                 max_batch=1, precision="f32", family=None):
        """precision: 'f32' (exact fp32 contractions, the parity path) or 'f16' (vit_48 contractions on f16 MFMA,
        BASELINE config 5).  The ViT-Base path (channels=768, heads=12) and the ViT-Large one (channels=1024, heads=16, head_channels=256
        at 128 / 256 or 192 / 384) always contract in bf16.
        family: None -- vt_create chooses the family from the widths (768 / 12 and the ViT-Large tuple: the patch-16 ViT; everything else,
        384 / 6 and 192 / 3 included, the LeViT-stem vit_dist model); "vit" -- vt_create_vit: the patch-16 OSTrack ViT at (channels, heads) =
        (192, 3) ViT-Tiny, (384, 6) ViT-Small, (768, 12), (1024, 16), anything else refused."""
        if family not in (None, "vit"):
            raise ValueError(f"family={family!r}: None (vt_create's choice) or 'vit'")
        self.precision, self.family = precision, family
        self._L = lib(precision)
        self.cfg = VtConfig(template_size, search_size, channels, heads, depth, head_channels, stride, max_batch)
        h = C.c_void_p()
        create = "vt_create_vit" if family == "vit" else "vt_create"
        _check(getattr(self._L, create)(C.byref(self.cfg), C.byref(h)), create, self._L)
        self._h = h
        q = [C.c_int32() for _ in range(4)]
        _check(self._L.vt_query(self._h, *[C.byref(v) for v in q]), "vt_query", self._L)
        self.len_z, self.len_x, self.feat_sz, self.channels = [v.value for v in q]
        self.L = self.len_z + self.len_x
        self.max_batch = max_batch
        self.template_size, self.search_size = template_size, search_size
        self._graphs = weakref.WeakSet()
        # the reference's torch float32 window, bit for bit (vt_create's libm one differs by ulps at F = 14, 16, 24)
        from .host_ops import hann2d
        self.set_window(hann2d((self.feat_sz, self.feat_sz)).numpy())

    def live_graphs(self) -> int:
        return sum(1 for g in self._graphs if g._valid)

    # ---- argument checks (raw device pointers cross the C ABI: a wrong shape would read out of bounds)
    def _check_crops(self, z, x):
        B = z.shape[0]
        tz, tx = self.template_size, self.search_size
        if tuple(z.shape) != (B, 3, tz, tz) or tuple(x.shape) != (B, 3, tx, tx):
            raise VtError(f"expected z (B,3,{tz},{tz}) and x (B,3,{tx},{tx}) with one batch size, got "
                          f"{tuple(z.shape)} and {tuple(x.shape)}")
        self._check_batch(B)
        return B

    def _check_batch(self, B):
        if not (1 <= B <= self.max_batch):
            raise VtError(f"batch {B} outside [1, max_batch={self.max_batch}]")

    def _check_out(self, out, B):
        F = self.feat_sz
        want = {"score_map": (B, 1, F, F), "size_map": (B, 2, F, F), "offset_map": (B, 2, F, F), "pred_boxes": (B, 4),
                "hann_boxes": (B, 4), "conf": (B,)}
        for k, shp in want.items():
            if tuple(getattr(out, k).shape) != shp:
                raise VtError(f"output buffer {k} has shape {tuple(getattr(out, k).shape)}, want {shp}")

    def close(self):
        for g in list(getattr(self, "_graphs", ())):
            g._invalidate()
        if getattr(self, "_h", None) and getattr(self, "_L", None) is not None:
            try:
                self._L.vt_destroy(self._h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self._h = None

    def __del__(self):
        self.close()

    def load_state_dict(self, sd: dict):
        """sd: name -> numpy array / torch tensor, reference ckpt['net'] layout (strict=False)."""
        keep, arr = [], (VtTensor * len(sd))()
        n = 0
        for k, v in sd.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            v = np.asarray(v)
            if v.dtype.kind != "f":
                continue   # num_batches_tracked etc.
            a = np.ascontiguousarray(v, dtype=np.float32)
            keep.append(a)
            arr[n] = VtTensor(k.encode(), a.ctypes.data, a.size)
            n += 1
        _check(self._L.vt_load_weights(self._h, arr, n), "vt_load_weights", self._L)

    def set_form_batch(self, n: int):
        """Choose the kernel forms as for a batch of n sequences (vt_set_form_batch): a shard of a group of n runs the forms the whole
        group would run, so a sequence's results do not depend on how the group is sharded.  0 = by each call's own batch."""
        _check(self._L.vt_set_form_batch(self._h, int(n)), "vt_set_form_batch", self._L)
        self.form_batch = int(n)

    def set_window(self, win):
        a = np.ascontiguousarray(np.asarray(win, dtype=np.float32).reshape(-1))
        if a.size != self.feat_sz ** 2:
            raise VtError(f"window must have {self.feat_sz ** 2} elements")
        _check(self._L.vt_set_window(self._h, a.ctypes.data), "vt_set_window", self._L)

    # ---- whole step
    def set_template(self, z, stream=None):
        """Exact template cache (vt_set_template): afterwards ``forward(None, x)`` / ``capture(None, x)`` skip the
        template's patch embedding and block 0's LayerNorm-1 + qkv of its rows.  On a ViT-Base / ViT-Large model (channels=768 / 1024) the cache holds the
        templates' bf16 patch-GEMM operand rows; forward(None, x), forward_u8(None, patch) and track_step* read it, bit-identical to the
        same call with z."""
        B, tz = z.shape[0], self.template_size
        if tuple(z.shape) != (B, 3, tz, tz):
            raise VtError(f"expected z (B,3,{tz},{tz}), got {tuple(z.shape)}")
        self._check_batch(B)
        _check(self._L.vt_set_template(self._h, _ptr(z), B, _stream(stream)), "vt_set_template", self._L)
        self._tmpl_B = B

    def _check_x_only(self, x):
        B, tx = x.shape[0], self.search_size
        if tuple(x.shape) != (B, 3, tx, tx):
            raise VtError(f"expected x (B,3,{tx},{tx}), got {tuple(x.shape)}")
        self._check_batch(B)
        if getattr(self, "_tmpl_B", 0) < B:
            raise VtError(f"forward with z=None needs set_template() for at least {B} frames first")
        return B

    def forward(self, z, x, out: Outputs | None = None, stream=None) -> Outputs:
        B = self._check_crops(z, x) if z is not None else self._check_x_only(x)
        out = out or Outputs(B, self.feat_sz, x.device)
        self._check_out(out, B)
        st = out.struct()
        _check(self._L.vt_forward(self._h, _ptr(z), _ptr(x), B, _stream(stream), C.byref(st)), "vt_forward", self._L)
        return out

    def capture(self, z, x, out: Outputs | None = None) -> tuple[Graph, Outputs]:
        B = self._check_crops(z, x) if z is not None else self._check_x_only(x)
        out = out or Outputs(B, self.feat_sz, x.device)
        self._check_out(out, B)
        st = out.struct()
        g = C.c_void_p()
        _check(self._L.vt_graph_capture(self._h, _ptr(z), _ptr(x), B, C.byref(st), C.byref(g)), "vt_graph_capture", self._L)
        gr = Graph(g, (z, x, out), self)
        self._graphs.add(gr)
        return gr, out

    def capture_steps(self, zs, xs, outs=None) -> tuple[Graph, list]:
        """``len(xs)`` consecutive steps in ONE graph: step i is ``forward(zs[i], xs[i], outs[i])``.  ``zs`` may be None (cached
        template) or hold None entries; steps run in order and may share tensors.  One launch then advances ``len(xs)`` frames --
        the gap the runtime leaves between two graph launches (~7 us) is paid once per graph instead of once per step."""
        n = len(xs)
        if n < 1:
            raise VtError("capture_steps needs at least one step")
        zs = list(zs) if zs is not None else [None] * n
        if len(zs) != n or (outs is not None and len(outs) != n):
            raise VtError("capture_steps: zs, xs and outs must have the same length")
        B = None
        for z, x in zip(zs, xs):
            b = self._check_crops(z, x) if z is not None else self._check_x_only(x)
            if B is not None and b != B:
                raise VtError("capture_steps: every step must have the same batch size")
            B = b
        outs = list(outs) if outs is not None else [Outputs(B, self.feat_sz, xs[0].device) for _ in range(n)]
        for o in outs:
            self._check_out(o, B)
        zp = (C.c_void_p * n)(*[_ptr(z) for z in zs])
        xp = (C.c_void_p * n)(*[_ptr(x) for x in xs])
        sts = (VtOutputs * n)(*[o.struct() for o in outs])
        g = C.c_void_p()
        _check(self._L.vt_graph_capture_steps(self._h, n, zp, xp, B, sts, C.byref(g)), "vt_graph_capture_steps", self._L)
        gr = Graph(g, (zs, list(xs), outs), self)
        self._graphs.add(gr)
        return gr, outs

    # ---- stages
    def stem(self, z, x, stream=None):
        import torch
        B = self._check_crops(z, x)
        tok = torch.empty(B, self.L, self.channels, device=z.device)
        _check(self._L.vt_stem(self._h, _ptr(z), _ptr(x), B, _stream(stream), _ptr(tok)), "vt_stem", self._L)
        return tok

    def blocks(self, tokens, nblocks=-1, want_resid=False, stream=None, feat=None):
        import torch
        B = tokens.shape[0]
        self._check_batch(B)
        if tuple(tokens.shape) != (B, self.L, self.channels):
            raise VtError(f"tokens must be (B,{self.L},{self.channels}), got {tuple(tokens.shape)}")
        if feat is None:
            feat = torch.empty(B, self.len_x, self.channels, device=tokens.device)
        elif tuple(feat.shape) != (B, self.len_x, self.channels):
            raise VtError(f"feat must be (B,{self.len_x},{self.channels}), got {tuple(feat.shape)}")
        resid = torch.empty_like(tokens) if want_resid else None
        _check(self._L.vt_blocks(self._h, _ptr(tokens), B, nblocks, _stream(stream), _ptr(feat), _ptr(resid)), "vt_blocks", self._L)
        return (feat, resid) if want_resid else feat

    def head(self, feat, out: Outputs | None = None, stream=None) -> Outputs:
        B = feat.shape[0]
        self._check_batch(B)
        if tuple(feat.shape) != (B, self.len_x, self.channels):
            raise VtError(f"feat must be (B,{self.len_x},{self.channels}), got {tuple(feat.shape)}")
        out = out or Outputs(B, self.feat_sz, feat.device)
        self._check_out(out, B)
        st = out.struct()
        _check(self._L.vt_head(self._h, _ptr(feat), B, _stream(stream), C.byref(st)), "vt_head", self._L)
        return out

    # ---- pre / post steps of track() on the device, from each of the three frame sources: a dense (B,H,W,3) batch, a frame table
    # (one frame of its own size per sequence, vt_*_frames), an image table (its own pixel format as well, vt_*_images)
    def _source(self, kind, src, B):
        """Entry-point suffix and leading arguments of a frame source for B sequences.  kind None: `src` is a dense (B,H,W,3) uint8
        tensor; kind FrameTable / ImageTable: a table of that class or a uint8 tensor holding its descriptors."""
        if kind is not None:
            return "_" + kind.KIND, (kind.ptr(src, B),)
        import torch
        if not ((src.is_cuda or src.is_pinned()) and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4
                and src.shape[3] == 3):
            raise VtError("frames must be a contiguous (B,H,W,3) uint8 tensor on the GPU (or in pinned host memory)")
        b, H, W, _ = src.shape
        if b != B:
            raise VtError(f"states must be ({b},4) for {b} frames (and so the step's crop workspace), got a batch of {B}")
        return "", (C.c_void_p(src.data_ptr()), H, W)

    def _table_args(self, states, out_shape, out_dtype, out, resize_factor):
        import torch
        if not (states.is_cuda and states.dtype == torch.float64 and states.is_contiguous() and states.dim() == 2 and states.shape[1] == 4):
            raise VtError("states must be a contiguous (B,4) float64 tensor on the GPU")
        B = int(states.shape[0])
        if out is None:
            out = torch.empty((B,) + out_shape, dtype=out_dtype, device=states.device)
        elif tuple(out.shape) != (B,) + out_shape or out.dtype != out_dtype or not out.is_cuda or not out.is_contiguous():
            raise VtError(f"crop output must be a contiguous {(B,) + out_shape} {out_dtype} tensor on the GPU")
        if resize_factor is None:
            resize_factor = torch.empty(B, dtype=torch.float64, device=states.device)
        elif tuple(resize_factor.shape) != (B,) or resize_factor.dtype != torch.float64 or not resize_factor.is_cuda:
            raise VtError(f"resize_factor must be a ({B},) float64 tensor on the GPU")
        return B, out, resize_factor

    def _crop(self, kind, src, states, factor, out_size, norm, out, resize_factor, stream):
        """vt_crop* (norm = (mean, std): the normalised fp32 crop) or vt_crop_u8* (norm = (): sample_target's uint8 patch) of a source."""
        import torch
        shape, dtype = ((3, out_size, out_size), torch.float32) if norm else ((out_size, out_size, 3), torch.uint8)
        B, out, resize_factor = self._table_args(states, shape, dtype, out, resize_factor)
        sfx, lead = self._source(kind, src, B)
        name = ("vt_crop" if norm else "vt_crop_u8") + sfx
        _check(getattr(self._L, name)(self._h, *lead, C.c_void_p(states.data_ptr()), float(factor), out_size, *map(_f3, norm), B,
                                      _stream(stream), C.c_void_p(out.data_ptr()), C.c_void_p(resize_factor.data_ptr())), name, self._L)
        return out, resize_factor

    def crop(self, frames, states, factor, out_size, mean, std, out=None, resize_factor=None, stream=None):
        """frames (B,H,W,3) uint8 cuda -- or PINNED host memory, which the kernel reads over the bus (a few sequences: no upload) --,
        states (B,4) float64 cuda -> (crops (B,3,T,T) fp32, resize_factor (B) fp64)."""
        return self._crop(None, frames, states, factor, out_size, (mean, std), out, resize_factor, stream)

    def crop_u8(self, frames, states, factor, out_size, out=None, resize_factor=None, stream=None):
        """sample_target alone (the uint8 patch path: its output goes to the stem as it is): frames (B,H,W,3) uint8 (GPU or pinned),
        states (B,4) float64 cuda -> (patch (B,T,T,3) uint8 -- the array the reference's sample_target returns --, resize_factor (B)
        fp64)."""
        return self._crop(None, frames, states, factor, out_size, (), out, resize_factor, stream)

    def crop_frames(self, table, states, factor, out_size, mean, std, out=None, resize_factor=None, stream=None):
        """crop() with a frame table (FrameTable / vt_crop_frames): sequence b is cropped from its own frame."""
        return self._crop(FrameTable, table, states, factor, out_size, (mean, std), out, resize_factor, stream)

    def crop_u8_frames(self, table, states, factor, out_size, out=None, resize_factor=None, stream=None):
        """crop_u8() with a frame table (vt_crop_u8_frames)."""
        return self._crop(FrameTable, table, states, factor, out_size, (), out, resize_factor, stream)

    def crop_images(self, table, states, factor, out_size, mean, std, out=None, resize_factor=None, stream=None):
        """crop_frames() on an image table (ImageTable / vt_crop_images): sequence b is cropped from rgb(images[b])."""
        return self._crop(ImageTable, table, states, factor, out_size, (mean, std), out, resize_factor, stream)

    def crop_u8_images(self, table, states, factor, out_size, out=None, resize_factor=None, stream=None):
        """crop_u8_frames() on an image table (vt_crop_u8_images)."""
        return self._crop(ImageTable, table, states, factor, out_size, (), out, resize_factor, stream)

    def _step(self, kind, src, states, factor, mean, std, x, resize_factor, out, record, margin, stream):
        """vt_track_step* on a source: the argument checks of the three public steps and the call."""
        import torch
        B = self._check_x_only(x)
        sfx, lead = self._source(kind, src, B)
        if (tuple(states.shape) != (B, 4) or states.dtype != torch.float64 or not states.is_cuda or not states.is_contiguous()
                or tuple(resize_factor.shape) != (B,) or resize_factor.dtype != torch.float64 or not resize_factor.is_cuda):
            raise VtError(f"track_step{sfx} wants states ({B},4) and resize_factor ({B},) float64 on the GPU")
        if record is not None and (tuple(record.shape) != (B, 5) or record.dtype != torch.float64 or not record.is_contiguous()
                                   or not (record.is_cuda or record.is_pinned())):
            raise VtError(f"record must be a contiguous ({B},5) float64 tensor on the GPU or in pinned host memory")
        self._check_out(out, B)
        st = out.struct()
        name = "vt_track_step" + sfx
        _check(getattr(self._L, name)(self._h, *lead, C.c_void_p(states.data_ptr()), float(factor), _f3(mean), _f3(std), B,
                                      _stream(stream), _ptr(x), C.c_void_p(resize_factor.data_ptr()), C.byref(st), margin,
                                      C.c_void_p(record.data_ptr()) if record is not None else None), name, self._L)
        return out

    def track_step(self, frames, states, factor, mean, std, x, resize_factor, out: Outputs, record=None, margin=10, stream=None):
        """crop -> network on the cached template -> map back / clip / state update (-> record) as ONE library call (vt_track_step):
        the same kernels as crop() + forward(None, x) + update_state_record(), with the tail fused into the decode kernel on the
        small-batch path.  frames (B,H,W,3) uint8 on the GPU or pinned; x: the (B,3,S,S) crop workspace; states (B,4) / resize_factor
        (B,) float64 on the GPU; record: optional (B,5) float64, GPU or pinned."""
        return self._step(None, frames, states, factor, mean, std, x, resize_factor, out, record, margin, stream)

    def track_step_frames(self, table, states, factor, mean, std, x, resize_factor, out: Outputs, record=None, margin=10, stream=None):
        """track_step() with a frame table (vt_track_step_frames): each sequence is cropped from, and clipped to, its own frame."""
        return self._step(FrameTable, table, states, factor, mean, std, x, resize_factor, out, record, margin, stream)

    def track_step_images(self, table, states, factor, mean, std, x, resize_factor, out: Outputs, record=None, margin=10, stream=None):
        """track_step_frames() on an image table (vt_track_step_images)."""
        return self._step(ImageTable, table, states, factor, mean, std, x, resize_factor, out, record, margin, stream)

    def set_template_slots(self, z, slots, stream=None):
        """Rewrite the template cache of the given slots only (vt_set_template_slots): z (n,3,Tz,Tz) fp32 on the GPU, slots n
        distinct indices below the cached batch.  Not capturable."""
        slots = [int(v) for v in slots]
        n = len(slots)
        if z is None or tuple(z.shape) != (n, 3, self.template_size, self.template_size):
            raise VtError(f"expected z ({n},3,{self.template_size},{self.template_size}) for {n} slots")
        arr = (C.c_int32 * max(n, 1))(*slots)
        _check(self._L.vt_set_template_slots(self._h, _ptr(z), arr, n, _stream(stream)), "vt_set_template_slots", self._L)

    def set_normalization(self, mean, std):
        """Preprocessor's mean / std for the uint8 entry points (folded into the stem's first layer; default: ImageNet)."""
        _check(self._L.vt_set_normalization(self._h, _f3(mean), _f3(std)), "vt_set_normalization", self._L)

    def set_candidate_elimination(self, loc, keep_ratio, template_rows=None, form=None):
        """OSTrack candidate elimination (vt_set_candidate_elimination): after block loc[k] the search tokens are ranked by the attention
        they receive from the selected template rows and ceil(keep_ratio[k] * kept so far) stay.  template_rows: (len_z,) booleans, None =
        every row.  form (vt_set_ce_form): "masked" -- removed tokens stay in place as absent keys -- or "compact" -- the kept tokens are
        gathered into shorter frames (ce_compact_lengths) behind every stage; None reads VB_CE_FORM and falls back to "masked".  Same
        results either way; the chosen form is ``ce_form``.  Before any capture; ViT-Base models only."""
        form = ce_form_name(form)
        loc, keep_ratio = [int(v) for v in loc], [float(v) for v in keep_ratio]
        if len(loc) != len(keep_ratio):
            raise VtError(f"candidate elimination: {len(loc)} blocks (CE_LOC) for {len(keep_ratio)} keep ratios (CE_KEEP_RATIO)")
        n = len(loc)
        rows = None
        if template_rows is not None:
            rows = np.ascontiguousarray(np.asarray(template_rows).reshape(-1) != 0, dtype=np.uint8)
            if rows.size != self.len_z:
                raise VtError(f"template_rows must have {self.len_z} entries, got {rows.size}")
        _check(self._L.vt_set_candidate_elimination(self._h, n, (C.c_int32 * max(n, 1))(*loc), (C.c_double * max(n, 1))(*keep_ratio),
                                                    rows.ctypes.data if rows is not None else None),
               "vt_set_candidate_elimination", self._L)
        _check(self._L.vt_set_ce_form(self._h, CE_FORMS[form]), "vt_set_ce_form", self._L)
        self.ce_form = form
        self.ce_stages = n
        self.ce_keep = ce_keep_counts(self.len_x, keep_ratio)

    def ce_result(self, B=None, stream=None):
        """(removed_stage (B, len_x) uint8: 0 = kept to the end, k = removed at stage k; scores (n, B, len_x) fp32: each stage's ranking
        score, NaN for tokens removed earlier) of the last forward / step / blocks call (vt_ce_result).  B: default max_batch."""
        import torch
        n = getattr(self, "ce_stages", 0)
        if not n:
            raise VtError("ce_result needs set_candidate_elimination() first")
        B = self.max_batch if B is None else int(B)
        self._check_batch(B)
        removed = torch.empty(B, self.len_x, dtype=torch.uint8, device="cuda")
        scores = torch.empty(n, B, self.len_x, dtype=torch.float32, device="cuda")
        _check(self._L.vt_ce_result(self._h, B, _stream(stream), C.c_void_p(removed.data_ptr()), C.c_void_p(scores.data_ptr())),
               "vt_ce_result", self._L)
        return removed, scores

    def set_open_loop(self, on: bool = True):
        """vt_set_open_loop: track_step (and graphs captured from now on) leave `states` untouched; the step's box is in `record`."""
        _check(self._L.vt_set_open_loop(self._h, 1 if on else 0), "vt_set_open_loop", self._L)

    def gemm_form(self, B: int) -> int:
        """vt_gemm_form: the GEMM_* bits of the GEMM kinds a plain forward of B frames runs on the narrow tile (0 on the vit_48 path)."""
        return int(self._L.vt_gemm_form(self._h, int(B)))

    def patch_u8_supported(self, B: int) -> bool:
        return bool(self._L.vt_patch_u8_supported(self._h, int(B)))

    def _check_patch(self, xp):
        import torch
        B, tx = xp.shape[0], self.search_size
        if tuple(xp.shape) != (B, tx, tx, 3) or xp.dtype != torch.uint8 or not xp.is_cuda or not xp.is_contiguous():
            raise VtError(f"expected a contiguous uint8 patch (B,{tx},{tx},3) on the GPU, got {tuple(xp.shape)} {xp.dtype}")
        self._check_batch(B)
        return B

    def forward_u8(self, z, x_patch, out: Outputs | None = None, stream=None) -> Outputs:
        """Preprocessor.process + forward on the uint8 search patch of crop_u8; z: fp32 template crop or None (cached template).
        ViT-Base and ViT-Large models take it at every batch size; the patch must be 16-byte aligned there (any torch allocation is)."""
        B = self._check_patch(x_patch)
        if z is None:
            if getattr(self, "_tmpl_B", 0) < B:
                raise VtError(f"forward_u8 with z=None needs set_template() for at least {B} frames first")
        elif tuple(z.shape) != (B, 3, self.template_size, self.template_size):
            raise VtError(f"expected z ({B},3,{self.template_size},{self.template_size}), got {tuple(z.shape)}")
        out = out or Outputs(B, self.feat_sz, x_patch.device)
        self._check_out(out, B)
        st = out.struct()
        _check(self._L.vt_forward_u8(self._h, _ptr(z), C.c_void_p(x_patch.data_ptr()), B, _stream(stream), C.byref(st)), "vt_forward_u8", self._L)
        return out

    def stem_u8(self, x_patch, tokens, stream=None):
        """Search rows of the token matrix from a uint8 patch (rows [len_z, L) of `tokens` (B,L,C) are written)."""
        B = self._check_patch(x_patch)
        if tuple(tokens.shape) != (B, self.len_z + self.len_x, self.channels):
            raise VtError(f"tokens must be ({B},{self.len_z + self.len_x},{self.channels}), got {tuple(tokens.shape)}")
        _check(self._L.vt_stem_u8(self._h, C.c_void_p(x_patch.data_ptr()), B, _stream(stream), _ptr(tokens)), "vt_stem_u8", self._L)
        return tokens

    def update_state(self, hann_boxes, resize_factor, states, search_size, H, W, margin=10, stream=None):
        B = states.shape[0]
        if (tuple(states.shape) != (B, 4) or tuple(hann_boxes.shape) != (B, 4) or tuple(resize_factor.shape) != (B,)
                or states.dtype != resize_factor.dtype or not states.is_cuda or not resize_factor.is_cuda):
            raise VtError(f"update_state wants hann_boxes ({B},4) fp32, resize_factor ({B},) fp64 and states ({B},4) fp64 "
                          f"on the GPU")
        _check(self._L.vt_update_state(self._h, _ptr(hann_boxes), C.c_void_p(resize_factor.data_ptr()), search_size, H, W,
                                     margin, B, _stream(stream), C.c_void_p(states.data_ptr())), "vt_update_state", self._L)
        return states

    def update_state_record(self, hann_boxes, conf, resize_factor, states, record, search_size, H, W, margin=10, stream=None):
        """update_state + the (B,5) float64 record [x, y, w, h, confidence] of the new state into `record`: a CUDA tensor or a
        PINNED host tensor (device-mapped: the kernel writes it over the bus, no copy afterwards)."""
        import torch
        B = states.shape[0]
        if (tuple(states.shape) != (B, 4) or tuple(hann_boxes.shape) != (B, 4) or tuple(resize_factor.shape) != (B,)
                or states.dtype != torch.float64 or resize_factor.dtype != torch.float64 or not states.is_cuda or not resize_factor.is_cuda):
            raise VtError(f"update_state_record wants hann_boxes ({B},4) fp32, resize_factor ({B},) fp64 and states ({B},4) fp64 on the GPU")
        if (tuple(record.shape) != (B, 5) or record.dtype != torch.float64 or not record.is_contiguous()
                or not (record.is_cuda or record.is_pinned())):
            raise VtError(f"record must be a contiguous ({B},5) float64 tensor on the GPU or in pinned host memory")
        _check(self._L.vt_update_state_record(self._h, _ptr(hann_boxes), _ptr(conf), C.c_void_p(resize_factor.data_ptr()), search_size,
                                            H, W, margin, B, _stream(stream), C.c_void_p(states.data_ptr()),
                                            C.c_void_p(record.data_ptr())), "vt_update_state_record", self._L)
        return record

    def cal_bbox(self, score, size, offset, stream=None):
        import torch
        B, F = score.shape[0], self.feat_sz
        if tuple(score.shape) != (B, 1, F, F) or tuple(size.shape) != (B, 2, F, F) or tuple(offset.shape) != (B, 2, F, F):
            raise VtError(f"cal_bbox wants (B,1,{F},{F}), (B,2,{F},{F}), (B,2,{F},{F}) maps, got {tuple(score.shape)}, "
                          f"{tuple(size.shape)}, {tuple(offset.shape)}")
        bbox = torch.empty(B, 4, device=score.device)
        mx = torch.empty(B, device=score.device)
        _check(self._L.vt_cal_bbox(self._h, _ptr(score), _ptr(size), _ptr(offset), B, _stream(stream), _ptr(bbox), _ptr(mx)),
               "vt_cal_bbox", self._L)
        return bbox, mx
