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

# the pixel formats of the image route live in pixfmt.py (no ctypes, no library); every public name of theirs is re-exported here
from .pixfmt import (ARENA_ALIGN, IMAGE_DTYPE, LAYOUTS, PIX_BGR, PIX_BGRA, PIX_BGRP, PIX_GRAY8, PIX_GRAY10, PIX_GRAY12,  # noqa: F401
                     PIX_GRAY16, PIX_I010, PIX_I012, PIX_I016, PIX_I210, PIX_I212, PIX_I216, PIX_I410, PIX_I412, PIX_I416, PIX_I420,
                     PIX_I422, PIX_I444, PIX_LAYOUT_NAMES, PIX_MATRICES, PIX_NAMES, PIX_NV12, PIX_NV16, PIX_NV21, PIX_NV24, PIX_P010,
                     PIX_P210, PIX_P410, PIX_RANGES, PIX_RGB, PIX_RGBA, PIX_RGBP, PIX_UYVY, PIX_YUYV, PIX_YV12, PIX_YV16, PIX_YV24,
                     WIDE_DEPTHS, WIDE_SUBS, Image, Layout, VtError, check_image, images_from_chw, pack_image_offsets, pack_planes,
                     pix_fields, pix_format, pix_name, pix_wide)

_HERE =os.path.dirname(os.path.abspath(__file__))
#: VITTRACK_LIB=<path> selects another build of the fp32 library (A/B tools: tools/ab_stages.py, tools/block_stamps.py)
LIB_PATH = os.environ.get("VITTRACK_LIB") or os.path.join(_HERE, "csrc", "libvittrack_hip.so")
#: the same sources built with every vit_48 contraction on f16 MFMA (BASELINE config 5; make -C csrc all)
LIB_PATH_F16 = os.path.join(_HERE, "csrc", "libvittrack_hip_f16.so")
PRECISIONS = ("f32", "f16")


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
    "vt_set_precision": (C.c_int, [_vp, _i32]),
    "vt_precision": (C.c_int, [_vp]),
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


class ImageTable(_DescriptorTable):
    """The (B,) vt_image descriptor table of vt_crop_images / vt_track_step_images (include/vittrack.h): one frame per sequence in
    its own pixel format, size and plane pitches."""

    DTYPE = IMAGE_DTYPE
    ITEM = IMAGE_DTYPE.itemsize
    KIND, WHAT = "images", "image table must be an ImageTable"

    #: check(fmt, ptr0, ptr1, H, W, pitch0=0, pitch1=0, reserved=0, nbytes0=None, nbytes1=None) -> the pitches used: the device's rules
    #: for an unusable descriptor, on the host, from the layout's row
    check = staticmethod(check_image)

    @staticmethod
    def check_descriptor(desc, nbytes0: int | None = None, nbytes1: int | None = None):
        """check() of a vt_image tuple (plane0, plane1, pitch0, pitch1, H, W, format, reserved)."""
        p0, p1, q0, q1, H, W, fmt, res = desc
        return check_image(fmt, p0, p1, H, W, q0, q1, res, nbytes0, nbytes1)

    def set(self, i: int, desc, keep=None, check: bool = True):
        """Entry i from a vt_image tuple (plane0, plane1, pitch0, pitch1, H, W, format, reserved); check=False writes it as it is."""
        p0, p1, q0, q1, H, W, fmt, res = desc = tuple(int(v) for v in desc)
        if check:
            q0, q1 = self.check_descriptor(desc)
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


#: the arithmetic modes of a patch-16 ViT model (include/vittrack.h VT_PRECISION_BF16 / VT_PRECISION_FP32)
VIT_PRECISIONS = {"bf16": 0, "fp32": 1}


def vit_precision_name(precision=None) -> str:
    """The mode's name: `precision`, or without one the environment variable VB_PRECISION, or "bf16"."""
    if precision is None:
        precision = os.environ.get("VB_PRECISION") or "bf16"
    if precision not in VIT_PRECISIONS:
        raise VtError(f"ViT precision {precision!r}: one of {sorted(VIT_PRECISIONS)}")
    return precision


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
        self.contractions, self.family = precision, family      # the library: 'f32' | 'f16'
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

    @property
    def precision(self) -> str:
        """A patch-16 ViT model: the arithmetic mode, "bf16" | "fp32" (vt_precision).  Any other model: the library's contractions,
        'f32' | 'f16', as the constructor took them."""
        v = int(self._L.vt_precision(self._h)) if getattr(self, "_h", None) else -1
        return self.contractions if v < 0 else ("bf16", "fp32")[v]

    def set_precision(self, precision: str):
        """vt_set_precision: "bf16" (single-piece bf16 operands, the default) or "fp32" (three-piece bf16 operands, six terms per product,
        fp32 activations: the reference's fp32 outputs to a few 1e-6).  Patch-16 ViT models only; not with candidate elimination; before
        any capture.  Allocates the mode's workspaces the first time; drops the template cache."""
        if precision not in VIT_PRECISIONS:
            raise VtError(f"ViT precision {precision!r}: one of {sorted(VIT_PRECISIONS)}")
        before = self.precision
        _check(self._L.vt_set_precision(self._h, VIT_PRECISIONS[precision]), "vt_set_precision", self._L)
        if before != precision:
            self._tmpl_B = 0      # the cache held the other mode's operand rows

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
