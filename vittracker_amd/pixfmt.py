"""Pixel formats of the image route (vt_image; vt_crop_images, vt_track_step_images): one row per layout in LAYOUTS, and everything the
host knows about a layout computed from its row -- the bytes and rows of each plane, which of H and W must be even, whether colour tags
are legal, how addresses and pitches must be aligned (check_image), and what the Image constructors ask of the planes they are given.

``image_view`` and ``yuv_layout`` in csrc/vt_track.h are the device's copy of the same rules; include/vittrack.h is the contract both
follow.  A new layout is one row here (and its constructor), one case there.

Needs neither ctypes nor the library, and imports torch only inside the functions that are handed tensors.  native.py re-exports every
public name of this module."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np


class VtError(RuntimeError):
    pass


#: struct vt_image (include/vittrack.h): {const uint8_t *plane0, *plane1; int64_t pitch0, pitch1; int32_t H, W, format, reserved;}
IMAGE_DTYPE = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("pitch0", "<i8"), ("pitch1", "<i8"), ("H", "<i4"), ("W", "<i4"),
                        ("format", "<i4"), ("reserved", "<i4")])
assert IMAGE_DTYPE.itemsize == 48
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


class Layout(NamedTuple):
    """One layout of bits 0-7 of vt_image.format."""
    code: int
    name: str
    planes: int                # planes the descriptor describes: 1, or 2 (plane 1 holds all the chroma, or the two trailing planes)
    bps: int                   # bytes a sample: 1, or 2 (little-endian 16-bit words)
    px: int                    # bytes a pixel in plane 0
    cshift: Optional[int]      # chroma columns are W >> cshift; None: no chroma (RGB and grey; planar RGB has 0, its trailing planes)
    rshift: int                # chroma rows are H >> rshift
    pairs: bool                # plane 1 holds (U, V) pairs; otherwise two planes of one pitch back to back
    colour: bool               # takes matrix / range bits
    align: int                 # 4: plane addresses are 4-byte aligned; 2: addresses and pitches even (16-bit loads); 1: read as bytes

    def row_bytes(self, W: int):
        """Bytes of one row of plane 0 and of plane 1 (0: no plane 1)."""
        return self.px * W, (self.bps * (W >> self.cshift) * (2 if self.pairs else 1) if self.planes == 2 else 0)

    def chroma_rows(self, H: int) -> int:
        """Rows of ONE chroma plane (a trailing plane begins pitch1 times this many bytes after plane 1)."""
        return H >> self.rshift

    def plane1_rows(self, H: int) -> int:
        """Rows of plane 1: a plane of pairs has the chroma rows, two planes back to back twice as many."""
        return (H >> self.rshift) * (1 if self.pairs else 2)


#: the 16-bit planar block of layout codes, 32 | sub << 2 | dep: sub 0 / 1 / 2 / 3 = 4:2:0 / 4:2:2 / 4:4:4 / luma only, dep 0 / 1 / 2 =
#: 10 / 12 / 16 bits in LSB-aligned words (dep 3 is never assigned)
WIDE_SUBS = ("420", "422", "444", "gray")
WIDE_DEPTHS = (10, 12, 16)


def pix_wide(sub: str, depth: int) -> int:
    """The layout code of a planar 16-bit layout: sub "420" | "422" | "444" | "gray", depth 10 | 12 | 16."""
    if sub not in WIDE_SUBS or depth not in WIDE_DEPTHS:
        raise VtError(f"a 16-bit planar layout is sub in {WIDE_SUBS} and depth in {WIDE_DEPTHS}, got {sub!r}, {depth!r}")
    return 32 | WIDE_SUBS.index(sub) << 2 | WIDE_DEPTHS.index(depth)


def _layouts():
    rows = [  # code, name, planes, bps, px, cshift, rshift, pairs, colour, align      (6, 7, 14, 15, 20, 27-31: never assigned)
        (0, "rgb", 1, 1, 3, None, 0, False, False, 4), (1, "bgr", 1, 1, 3, None, 0, False, False, 4),
        (2, "rgba", 1, 1, 4, None, 0, False, False, 4), (3, "bgra", 1, 1, 4, None, 0, False, False, 4),
        (4, "nv12", 2, 1, 1, 1, 1, True, True, 4), (5, "nv21", 2, 1, 1, 1, 1, True, True, 4),
        (8, "i420", 2, 1, 1, 1, 1, False, True, 4), (9, "yv12", 2, 1, 1, 1, 1, False, True, 4),
        (10, "yuyv", 1, 1, 2, 1, 0, False, True, 4), (11, "uyvy", 1, 1, 2, 1, 0, False, True, 4),
        (12, "p010", 2, 2, 2, 1, 1, True, True, 4), (13, "gray8", 1, 1, 1, None, 0, False, False, 4),
        # three full-height planes of single bytes, and the two-plane 4:2:2 / 4:4:4 layouts (P210 / P410: MSB-aligned words, read through
        # their high byte): any address
        (16, "rgbp", 2, 1, 1, 0, 0, False, False, 1), (17, "bgrp", 2, 1, 1, 0, 0, False, False, 1),
        (18, "i444", 2, 1, 1, 0, 0, False, True, 1), (19, "i422", 2, 1, 1, 1, 0, False, True, 1),
        (21, "yv16", 2, 1, 1, 1, 0, False, True, 1), (22, "yv24", 2, 1, 1, 0, 0, False, True, 1),
        (23, "nv16", 2, 1, 1, 1, 0, True, True, 1), (24, "nv24", 2, 1, 1, 0, 0, True, True, 1),
        (25, "p210", 2, 2, 2, 1, 0, True, True, 1), (26, "p410", 2, 2, 2, 0, 0, True, True, 1)]
    # the planar 16-bit block: 10- and 12-bit words are fetched as aligned 16-bit loads, the 16-bit depth through its high byte
    shifts = {"420": ("i0", 1, 1), "422": ("i2", 1, 0), "444": ("i4", 0, 0), "gray": ("gray", None, 0)}
    for sub, (stem, cs, rs) in shifts.items():
        rows += [(pix_wide(sub, d), f"{stem}{d}", 1 if cs is None else 2, 2, 2, cs, rs, False, cs is not None, 2 if d < 16 else 1) for d in WIDE_DEPTHS]
    return {r[0]: Layout(*r) for r in rows}


#: layout code -> its row
LAYOUTS = _layouts()
#: layout code -> lower-case name
PIX_LAYOUT_NAMES = {c: L.name for c, L in LAYOUTS.items()}
#: vt_image.format (include/vittrack.h), bits 0-7 ...
PIX_RGB, PIX_BGR, PIX_RGBA, PIX_BGRA, PIX_NV12, PIX_NV21 = range(6)
PIX_NAMES = tuple(PIX_LAYOUT_NAMES[c] for c in range(6))
PIX_I420, PIX_YV12, PIX_YUYV, PIX_UYVY, PIX_P010, PIX_GRAY8 = range(8, 14)
PIX_RGBP, PIX_BGRP, PIX_I444, PIX_I422 = range(16, 20)
PIX_YV16, PIX_YV24, PIX_NV16, PIX_NV24, PIX_P210, PIX_P410 = range(21, 27)
PIX_I010, PIX_I012, PIX_I016 = (pix_wide("420", d) for d in WIDE_DEPTHS)
PIX_I210, PIX_I212, PIX_I216 = (pix_wide("422", d) for d in WIDE_DEPTHS)
PIX_I410, PIX_I412, PIX_I416 = (pix_wide("444", d) for d in WIDE_DEPTHS)
PIX_GRAY10, PIX_GRAY12, PIX_GRAY16 = (pix_wide("gray", d) for d in WIDE_DEPTHS)
#: ... its bits 8-11 (the matrix of a YUV layout) and 12-15 (its range); bits 16-31 must be 0
PIX_MATRICES = ("bt601", "bt709")
PIX_RANGES = ("limited", "full")


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


def check_image(fmt: int, ptr0: int, ptr1: int, H: int, W: int, pitch0: int = 0, pitch1: int = 0, reserved: int = 0,
                nbytes0: int | None = None, nbytes1: int | None = None):
    """The device's rules for an unusable descriptor, on the host: raises VtError where the kernels would poison the sequence.
    Returns the pitches actually used (0 -> the row's bytes).  nbytes0 / nbytes1: bytes available from each plane (buffers)."""
    fmt, H, W, pitch0, pitch1 = int(fmt), int(H), int(W), int(pitch0), int(pitch1)
    lay, mat, rng, high = pix_fields(fmt)
    L = LAYOUTS.get(lay)
    if L is None:
        raise VtError(f"unknown pixel format {fmt}")
    if high or mat >= len(PIX_MATRICES) or rng >= len(PIX_RANGES):
        raise VtError(f"unknown pixel format {fmt:#x}: matrix {mat}, range {rng}, bits 16-31 {high:#x}")
    if (mat or rng) and not L.colour:
        raise VtError(f"a {pix_name(fmt)} image takes no matrix or range bits, got format {fmt:#x}")
    if int(reserved) != 0:
        raise VtError("vt_image.reserved must be 0")
    if H < 1 or W < 1 or H > 0x10000000 or W > 0x10000000:
        raise VtError(f"image of {H}x{W} pixels: H and W must be >= 1")
    if L.rshift and (H % 2 or W % 2):      # every layout of halved chroma rows has halved chroma columns
        raise VtError(f"an {pix_name(fmt)} image must have even H and W, got {H}x{W}")
    if L.cshift and W % 2:
        raise VtError(f"a {pix_name(fmt)} image must have even W, got {H}x{W}")
    r0, r1 = L.row_bytes(W)
    planes = [(ptr0, pitch0, H, r0, nbytes0)] + ([(ptr1, pitch1, L.plane1_rows(H), r1, nbytes1)] if r1 else [])
    used = []
    for k, (ptr, pitch, rows, rb, nb) in enumerate(planes):
        pitch = pitch or rb
        if pitch < rb:
            raise VtError(f"plane {k}: row pitch {pitch} is shorter than a row ({rb} bytes)")
        if not ptr or (L.align == 4 and int(ptr) % 4):
            raise VtError(f"plane {k}: address {int(ptr or 0):#x} is null or not 4-byte aligned")
        if L.align == 2 and (int(ptr) % 2 or pitch % 2):
            raise VtError(f"plane {k}: address {int(ptr):#x} or row pitch {pitch} is odd; the 16-bit samples of a {pix_name(fmt)} image "
                          f"must be 2-byte aligned")
        need = pitch * (rows - 1) + rb
        if pitch > 0xfffffff0 or need > 0xfffffff0:
            raise VtError(f"plane {k}: {need} bytes are beyond the 32-bit offsets of the crop kernels")
        if nb is not None and need > int(nb):
            raise VtError(f"plane {k}: needs {need} bytes, its buffer has {int(nb)}")
        used.append(pitch)
    return used[0], (used[1] if len(used) > 1 else pitch1)      # a one-plane layout: ptr1 is not looked at, pitch1 comes back as given


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

    @staticmethod
    def _address(a) -> int:
        return int(a.data_ptr()) if hasattr(a, "data_ptr") else int(a.__array_interface__["data"][0])

    # ---- one plane validator ... ---------------------------------------------------------------------------------------------------
    @classmethod
    def _plane(cls, a, shape, name, what):
        """(row pitch, on the GPU) of one plane, which must be uint8 of `shape` = (rows, columns) or (rows, items, bytes an item) with
        every row's bytes contiguous and rows at least a row apart.  A plane of one row takes its pitch from the row's bytes."""
        got, st, gpu = cls._strides(a)
        if tuple(got) != tuple(shape):
            raise VtError(f"{name} {what} must be {tuple(shape)} bytes, got {tuple(got)}")
        rows, rb = shape[0], shape[1] * (shape[2] if len(shape) == 3 else 1)
        if (len(shape) == 3 and st[2] != 1) or (shape[1] > 1 and st[1] != rb // shape[1]) or (rows > 1 and st[0] < rb):
            raise VtError(f"{name} {what} strides {tuple(st)}: the {rb} bytes of a row must be contiguous, rows at least that far apart")
        return (st[0] if rows > 1 else rb), gpu

    @staticmethod
    def _hw(a, L, what, item=()):
        """(H, W) of a layout from plane 0, (H, W * bytes a sample) + item bytes: both >= 1, even where the layout halves the chroma."""
        shape = tuple(getattr(a, "shape", ()))
        even = " with H and W even" if L.rshift else " with W even" if L.cshift else ""
        if len(shape) != 2 + len(item) or shape[2:] != item or shape[0] < 1 or shape[1] < L.bps or shape[1] % L.bps \
                or (L.cshift and shape[1] // L.bps % 2) or (L.rshift and shape[0] % 2):
            raise VtError(f"{L.name.upper()} {what} must be (H, W{''.join(f', {n}' for n in item)}){even}"
                          f"{' in 16-bit samples' if L.bps == 2 else ''}, got {shape}")
        return int(shape[0]), int(shape[1]) // L.bps

    # ---- ... and three assemblers --------------------------------------------------------------------------------------------------
    @classmethod
    def _one(cls, fmt, a):
        """One plane: packed pixels (H, W, bytes a pixel), or samples (H, W * bytes a sample)."""
        L = LAYOUTS[fmt & 0xff]
        item = (L.px,) if L.px > L.bps else ()
        H, W = cls._hw(a, L, "image", item)
        return cls(fmt, (a,), H, W, (cls._plane(a, (H, W * L.bps) + item, L.name.upper(), "image")[0],))

    @classmethod
    def _two(cls, fmt, y, c):
        """Luma (H, W) and a plane of (U, V) pairs (chroma rows, chroma columns, 2), in bytes a sample."""
        L = LAYOUTS[fmt & 0xff]
        name = L.name.upper()
        H, W = cls._hw(y, L, "luma plane")
        q0, g0 = cls._plane(y, (H, W * L.bps), name, "luma plane")
        q1, g1 = cls._plane(c, (H >> L.rshift, W >> L.cshift, 2 * L.bps), name, "chroma plane")
        if g0 != g1:
            raise VtError(f"the two planes of an {name} image must both be on the GPU or both on the host")
        return cls(fmt, (y, c), H, W, (q0, q1))

    @classmethod
    def _three(cls, fmt, p0, p1, p2, apart_on_host=False):
        """Plane 0 (H, W) and two trailing planes (chroma rows, chroma columns), in bytes a sample.  The descriptor has two plane
        pointers and two pitches: the trailing planes must share one row pitch and the third must begin pitch1 * (its rows) bytes after
        the second; with one row, the pitch is what lies between them.  Planes that lie otherwise raise; nothing is copied here.
        apart_on_host (I420 / YV12): host planes may lie anywhere, host_planes() stacks them."""
        L = LAYOUTS[fmt & 0xff]
        name = L.name.upper()
        H, W = cls._hw(p0, L, "first plane")
        ch, cw = L.chroma_rows(H), (W >> L.cshift) * L.bps
        q0, g0 = cls._plane(p0, (H, W * L.bps), name, "first plane")
        (qa, ga), (qb, gb) = (cls._plane(p, (ch, cw), name, "trailing plane") for p in (p1, p2))
        if not g0 == ga == gb:
            raise VtError(f"the planes of an {name} image must all be on the GPU or all on the host")
        if qa != qb:
            raise VtError(f"the two trailing planes of an {name} image must have one row pitch, got {qa} and {qb}")
        gap = cls._address(p2) - cls._address(p1)
        pitch1 = qa if ch > 1 or apart_on_host else gap
        if (g0 or not apart_on_host) and (gap != pitch1 * ch or pitch1 < cw):
            raise VtError(f"the trailing planes of an {name} image are {'not contiguous' if apart_on_host else 'not back to back'}: the third "
                          f"must begin pitch1 * {ch} rows = {pitch1 * ch} bytes after the second, it begins {gap} bytes after it (the descriptor "
                          f"has one pointer and one pitch for both); put them into one buffer, e.g. Image.i420_buffer or a (3, H, W) array for Image.chw")
        return cls(fmt, (p0, p1, p2), H, W, (q0, pitch1))

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
    def _wide(cls, assemble, lay, matrix, range, *planes):      # noqa: A002
        """A constructor of 16-bit planes: the assembler over their byte views."""
        return assemble(pix_format(lay, matrix, range), *(cls._bytes16(p, "luma" if k == 0 else "chroma", pix_name(lay)) for k, p in enumerate(planes)))

    # ---- the constructors ----------------------------------------------------------------------------------------------------------
    @classmethod
    def rgb(cls, a):
        return cls._one(PIX_RGB, a)

    @classmethod
    def bgr(cls, a):
        """A BGR frame as OpenCV hands it out (cv.imread, cv.VideoCapture)."""
        return cls._one(PIX_BGR, a)

    @classmethod
    def rgba(cls, a):
        return cls._one(PIX_RGBA, a)

    @classmethod
    def bgra(cls, a):
        return cls._one(PIX_BGRA, a)

    @classmethod
    def gray(cls, a):
        """An 8-bit grey frame (thermal / IR cameras), (H, W): rgb = (Y, Y, Y), no conversion."""
        return cls._one(PIX_GRAY8, a)

    @classmethod
    def nv12(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A decoder's NV12 surface: luma (H, W) and interleaved (U, V) pairs (H/2, W/2, 2)."""
        return cls._two(pix_format(PIX_NV12, matrix, range), y, uv)

    @classmethod
    def nv21(cls, y, vu, matrix="bt601", range="limited"):      # noqa: A002
        """NV21: as NV12 with (V, U) pairs."""
        return cls._two(pix_format(PIX_NV21, matrix, range), y, vu)

    @classmethod
    def p010(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A 10-bit decoder's P010 surface (a P016 one is read the same way): NV12's layout in little-endian 16-bit samples -- luma
        (H, W) and (U, V) pairs (H/2, W/2, 2) as uint16 / int16 arrays or tensors, or their uint8 views (H, 2 W) and (H/2, W/2, 4).
        The 8-bit sample is the high byte of each word."""
        return cls._wide(cls._two, PIX_P010, matrix, range, y, uv)

    @classmethod
    def i420(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:2:0 as software decoders produce it (ffmpeg's yuv420p): luma (H, W), U and V (H/2, W/2) each.  On the GPU the V
        plane must begin pitch1 * H/2 bytes after the U plane; host planes are packed that way into the arena."""
        return cls._three(pix_format(PIX_I420, matrix, range), y, u, v, apart_on_host=True)

    @classmethod
    def yv12(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV12: I420 with the V plane first."""
        return cls._three(pix_format(PIX_YV12, matrix, range), y, v, u, apart_on_host=True)

    @classmethod
    def i420_buffer(cls, buf, matrix="bt601", range="limited"):      # noqa: A002
        """One contiguous I420 buffer as OpenCV (COLOR_YUV2RGB_I420) and av_image_copy_to_buffer lay it out: a (3H/2, W) array of tight
        rows -- H rows of luma, then the U plane, then the V plane (H/2 rows of W/2 bytes each)."""
        shape = tuple(getattr(buf, "shape", ()))
        if len(shape) != 2 or shape[0] < 3 or shape[0] % 3 or shape[1] < 2 or shape[1] % 2:
            raise VtError(f"an I420 buffer must be (3H/2, W) with H and W even, got {shape}")
        H, W = 2 * int(shape[0]) // 3, int(shape[1])
        if cls._plane(buf, shape, "I420", "buffer")[0] != W:
            raise VtError(f"I420 buffer strides {cls._strides(buf)[1]}: rows must be tight (W bytes apart), the chroma planes follow the luma plane")
        c = buf[H:].reshape(H, W // 2)      # both chroma planes, H / 2 rows each: a view
        return cls(pix_format(PIX_I420, matrix, range), (buf[:H], c), H, W, (W, W // 2))

    @classmethod
    def yuyv(cls, a, matrix="bt601", range="limited"):      # noqa: A002
        """Packed 4:2:2 as capture cards and webcams produce it (YUY2): (H, W, 2), each 4 bytes Y0 U Y1 V."""
        return cls._one(pix_format(PIX_YUYV, matrix, range), a)

    @classmethod
    def uyvy(cls, a, matrix="bt601", range="limited"):      # noqa: A002
        """UYVY: each 4 bytes U Y0 V Y1."""
        return cls._one(pix_format(PIX_UYVY, matrix, range), a)

    @classmethod
    def yv16(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV16: I422 with the V plane first; U begins pitch1 * H bytes after V."""
        return cls._three(pix_format(PIX_YV16, matrix, range), y, v, u)

    @classmethod
    def yv24(cls, y, v, u, matrix="bt601", range="limited"):      # noqa: A002
        """YV24: I444 with the V plane first."""
        return cls._three(pix_format(PIX_YV24, matrix, range), y, v, u)

    @classmethod
    def nv16(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """Two-plane 4:2:2 as capture cards produce it: luma (H, W) and (U, V) pairs (H, W/2, 2); W even."""
        return cls._two(pix_format(PIX_NV16, matrix, range), y, uv)

    @classmethod
    def nv24(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """Two-plane 4:4:4: luma (H, W) and (U, V) pairs (H, W, 2)."""
        return cls._two(pix_format(PIX_NV24, matrix, range), y, uv)

    @classmethod
    def p210(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """A hardware decoder's P210 surface (a P216 one is read the same way): NV16 in little-endian 16-bit samples, as uint16 /
        int16 arrays or tensors (H, W) and (H, W/2, 2), or their uint8 views.  The 8-bit sample is the high byte of each word."""
        return cls._wide(cls._two, PIX_P210, matrix, range, y, uv)

    @classmethod
    def p410(cls, y, uv, matrix="bt601", range="limited"):      # noqa: A002
        """P410 / P416: NV24 in little-endian 16-bit samples, (H, W) and (H, W, 2); the high byte of each word."""
        return cls._wide(cls._two, PIX_P410, matrix, range, y, uv)

    @classmethod
    def yuv16(cls, y, u, v, depth=10, sub="420", matrix="bt601", range="limited"):      # noqa: A002
        """Planar YUV in LSB-aligned little-endian 16-bit samples (ffmpeg's yuv420p10le ... yuv444p16le): depth 10 | 12 | 16, sub "420"
        | "422" | "444"; luma (H, W), U and V (H/2, W/2), (H, W/2) or (H, W) as uint16 / int16 arrays or tensors, or their uint8 views
        (last axis doubled).  The 8-bit sample is min(word >> (depth - 8), 255).  V must begin pitch1 * (chroma rows) bytes after U;
        10- and 12-bit planes must lie at even addresses and even pitches (they are fetched as 16-bit words)."""
        if sub not in WIDE_SUBS[:3]:
            raise VtError(f"sub must be one of {WIDE_SUBS[:3]}, got {sub!r}")
        return cls._wide(cls._three, pix_wide(sub, depth), matrix, range, y, u, v)

    @classmethod
    def i010(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """yuv420p10le, what software HEVC Main10 / AV1 10-bit decoders produce: Image.yuv16(y, u, v, depth=10, sub="420")."""
        return cls.yuv16(y, u, v, 10, "420", matrix, range)

    @classmethod
    def gray16(cls, a, depth=16):
        """A grey frame in LSB-aligned little-endian 16-bit samples (gray10le / gray12le / gray16le; thermal and scientific cameras),
        (H, W) uint16 / int16 or its uint8 view (H, 2 W): rgb = (s, s, s) with s = min(word >> (depth - 8), 255)."""
        lay = pix_wide("gray", depth)
        return cls._one(lay, cls._bytes16(a, "plane", pix_name(lay)))

    @classmethod
    def rgb_planar(cls, r, g, b):
        """Planar RGB: three (H, W) planes.  G and B must share one row pitch with B beginning pitch * H bytes after G (the planes of a
        (3, H, W) array lie so); R may be anywhere."""
        return cls._three(PIX_RGBP, r, g, b)

    @classmethod
    def bgr_planar(cls, b, g, r):
        """Planar BGR: as rgb_planar with the B plane first."""
        return cls._three(PIX_BGRP, b, g, r)

    @classmethod
    def i444(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:4:4 (ffmpeg's yuv444p; screen capture): luma, U and V, (H, W) each; V begins pitch1 * H bytes after U."""
        return cls._three(pix_format(PIX_I444, matrix, range), y, u, v)

    @classmethod
    def i422(cls, y, u, v, matrix="bt601", range="limited"):      # noqa: A002
        """Planar 4:2:2 (yuv422p): luma (H, W), U and V (H, W/2) each, W even; V begins pitch1 * H bytes after U."""
        return cls._three(pix_format(PIX_I422, matrix, range), y, u, v)

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
            return cls._one(PIX_RGB if order == "rgb" else PIX_BGR, t.permute(1, 2, 0) if hasattr(t, "permute") else t.transpose(1, 2, 0))
        if shape[2] > 1 and st[2] != 1:
            raise VtError(f"CHW strides {tuple(st)}: the last dimension must be dense (or the view a permuted (H, W, 3) array)")
        return cls._three(PIX_RGBP if order == "rgb" else PIX_BGRP, t[0], t[1], t[2])

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
        L = LAYOUTS[self.format & 0xff]
        r0, r1 = L.row_bytes(self.W)
        return [(self.H, r0)] + ([(L.plane1_rows(self.H), r1)] if r1 else [])

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
