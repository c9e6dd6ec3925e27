"""numpy oracle of rgb(d) for the planar layouts of vt_image (include/vittrack.h): RGBP / BGRP (planar RGB, the CHW tensors of PyTorch
dataloaders), I444 and I422.  Written from the header's table alone, int64 throughout, on planes of arbitrary row pitches: no product
code.  The colour arithmetic and its four coefficient rows are tests/pixel_oracle_yuv.py's; chroma is never interpolated (I444: every
pixel its own U, V; I422: the pair x >> 1 shares them)."""
import numpy as np

from pixel_oracle_yuv import COLOURS, yuv_to_rgb

PLANAR_LAYOUTS = ("rgbp", "bgrp", "i444", "i422")
PLANAR_YUV = ("i444", "i422")
LAYOUT_CODE = {"rgbp": 16, "bgrp": 17, "i444": 18, "i422": 19}
#: every legal (layout, matrix, range): the four colour rows on I444 / I422, none on planar RGB
COMBOS = [(lay, "bt601", "limited") for lay in ("rgbp", "bgrp")] + [(lay, m, r) for lay in PLANAR_YUV for (m, r) in COLOURS]


def format_word(layout, matrix="bt601", rng="limited"):
    return LAYOUT_CODE[layout] | (("bt601", "bt709").index(matrix) << 8) | (("limited", "full").index(rng) << 12)


def chroma_width(layout, W):
    return W // 2 if layout == "i422" else W


def plane_bytes(buf, offset, pitch, rows, cols):
    """The (rows, cols) bytes of a plane that begins `offset` bytes into the flat uint8 buffer `buf`, rows `pitch` bytes apart: read
    byte by byte as the header describes a plane, int64."""
    buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
    idx = offset + pitch * np.arange(rows, dtype=np.int64)[:, None] + np.arange(cols, dtype=np.int64)[None, :]
    return buf[idx].astype(np.int64)


def rgb_of_buffers(layout, buf0, pitch0, buf1, pitch1, H, W, matrix="bt601", rng="limited", off0=0, off1=0):
    """rgb(d) of a descriptor: plane0 at buf0[off0:] with pitch0; plane1 at buf1[off1:] with pitch1, the third plane pitch1 * H bytes
    after it."""
    cw = chroma_width(layout, W)
    a = plane_bytes(buf0, off0, pitch0, H, W)
    b = plane_bytes(buf1, off1, pitch1, H, cw)
    c = plane_bytes(buf1, off1 + pitch1 * H, pitch1, H, cw)
    if layout == "rgbp":
        return np.stack([a, b, c], axis=-1).astype(np.uint8)
    if layout == "bgrp":
        return np.stack([c, b, a], axis=-1).astype(np.uint8)
    x = np.arange(W)
    cx = x >> 1 if layout == "i422" else x
    return yuv_to_rgb(a, b[:, cx], c[:, cx], matrix, rng)


def rgb_of(layout, planes, matrix="bt601", rng="limited"):
    """rgb(d) of a layout name and its three tight planes (as random_planes makes them)."""
    p0, p1, p2 = (np.ascontiguousarray(p) for p in planes)
    H, W = p0.shape
    cw = chroma_width(layout, W)
    assert p1.shape == p2.shape == (H, cw), (layout, p0.shape, p1.shape, p2.shape)
    return rgb_of_buffers(layout, p0, W, np.concatenate([p1, p2], axis=0), cw, H, W, matrix, rng)


def random_planes(rs, layout, H, W):
    """Three random tight planes of an H x W image in the shapes the Image constructors take."""
    r8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    cw = chroma_width(layout, W)
    return [r8(H, W), r8(H, cw), r8(H, cw)]
