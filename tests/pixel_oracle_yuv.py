"""numpy oracle of rgb(d) for the layouts and colour rows added to vt_image (include/vittrack.h): I420 / YV12, YUYV / UYVY, P010, GRAY8
and NV12 / NV21, each YUV layout under BT.601 / BT.709 and limited / full range.  Written from the header's formulas alone, int64
throughout: no product code.  Chroma is never interpolated: every pixel takes the one (U, V) its 2 x 2 (4:2:0) or 2 x 1 (4:2:2)
block shares."""
import numpy as np

#: (matrix, range) -> (cy, cvr, cvg, cug, cub): round(x 2^20) of the exact rationals; the 601-limited row is OpenCV's literals
COEF = {
    ("bt601", "limited"): (1220542, 1673527, 852492, 409993, 2116026),
    ("bt601", "full"): (1048576, 1470104, 748826, 360853, 1858077),
    ("bt709", "limited"): (1220945, 1879825, 558796, 223607, 2215014),
    ("bt709", "full"): (1048576, 1651297, 490864, 196424, 1945738),
}
COLOURS = tuple(COEF)
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
YUV_LAYOUTS = ("nv12", "nv21", "i420", "yv12", "yuyv", "uyvy", "p010")
NEW_LAYOUTS = ("i420", "yv12", "yuyv", "uyvy", "p010", "gray")
#: vt_image.format: layout in bits 0-7, matrix in bits 8-11, range in bits 12-15
LAYOUT_CODE = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3, "nv12": 4, "nv21": 5, "i420": 8, "yv12": 9, "yuyv": 10, "uyvy": 11, "p010": 12,
               "gray": 13}


def format_word(layout, matrix="bt601", rng="limited"):
    return LAYOUT_CODE[layout] | (("bt601", "bt709").index(matrix) << 8) | (("limited", "full").index(rng) << 12)


def fixed_point(Y, U, V, matrix="bt601", rng="limited"):
    """The three channels BEFORE the shift and the clamp, int64 (..., 3)."""
    cy, cvr, cvg, cug, cub = COEF[(matrix, rng)]
    Y, U, V = (np.asarray(a, dtype=np.int64) for a in (Y, U, V))
    yy = (np.maximum(Y - 16, 0) if rng == "limited" else Y) * cy
    u, v = U - 128, V - 128
    return np.stack([yy + cvr * v + (1 << 19), yy - cvg * v - cug * u + (1 << 19), yy + cub * u + (1 << 19)], axis=-1)


def yuv_to_rgb(Y, U, V, matrix="bt601", rng="limited"):
    """int arrays of equal shape -> (..., 3) uint8; numpy's >> on a negative int64 is arithmetic."""
    return np.clip(fixed_point(Y, U, V, matrix, rng) >> 20, 0, 255).astype(np.uint8)


def truth_fp64(Y, U, V, matrix, rng):
    """The fp64 formula, unclamped: luma scale 255/219 (limited) or 1, chroma scale 255/224 or 1 on 2(1-Kr), 2(1-Kr)Kr/Kg,
    2(1-Kb)Kb/Kg, 2(1-Kb)."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ls, cs = (255.0 / 219.0, 255.0 / 224.0) if rng == "limited" else (1.0, 1.0)
    Y, U, V = (np.asarray(a, dtype=np.float64) for a in (Y, U, V))
    yy = (np.maximum(Y - 16.0, 0.0) if rng == "limited" else Y) * ls
    u, v = U - 128.0, V - 128.0
    return np.stack([yy + cs * 2 * (1 - kr) * v, yy - cs * 2 * (1 - kr) * kr / kg * v - cs * 2 * (1 - kb) * kb / kg * u,
                     yy + cs * 2 * (1 - kb) * u], axis=-1)


def _up(a, fy, fx):
    return np.repeat(np.repeat(np.asarray(a), fy, axis=0), fx, axis=1)


def rgb_of(layout, planes, matrix="bt601", rng="limited"):
    """rgb(d) of a layout name and its planes (numpy, as random_planes makes them)."""
    if layout == "gray":
        return np.ascontiguousarray(np.repeat(np.asarray(planes[0])[..., None], 3, axis=2))
    if layout in ("nv12", "nv21"):
        y, c = planes
        U, V = (c[..., 1], c[..., 0]) if layout == "nv21" else (c[..., 0], c[..., 1])
        return yuv_to_rgb(y, _up(U, 2, 2), _up(V, 2, 2), matrix, rng)
    if layout == "p010":      # little-endian 16-bit samples: the 8-bit sample is the high byte
        y, c = (np.asarray(p).astype(np.uint16) >> 8 for p in planes)
        return yuv_to_rgb(y, _up(c[..., 0], 2, 2), _up(c[..., 1], 2, 2), matrix, rng)
    if layout in ("i420", "yv12"):
        y, a, b = planes
        U, V = (b, a) if layout == "yv12" else (a, b)
        return yuv_to_rgb(y, _up(U, 2, 2), _up(V, 2, 2), matrix, rng)
    if layout in ("yuyv", "uyvy"):
        p = np.asarray(planes[0])      # (H, W, 2): each 4 bytes Y0 U Y1 V or U Y0 V Y1
        yi, ci = (0, 1) if layout == "yuyv" else (1, 0)
        return yuv_to_rgb(p[..., yi], _up(p[:, 0::2, ci], 1, 2), _up(p[:, 1::2, ci], 1, 2), matrix, rng)
    raise ValueError(layout)


def random_planes(rs, layout, H, W):
    """Random planes of an H x W image (numpy, tight), in the shapes the Image constructors take."""
    r8 = lambda *s: rs.randint(0, 256, s).astype(np.uint8)      # noqa: E731
    if layout == "gray":
        return [r8(H, W)]
    if layout in ("nv12", "nv21"):
        return [r8(H, W), r8(H // 2, W // 2, 2)]
    if layout == "p010":      # every bit random, the low byte included (P016 surfaces): it must not reach the result
        return [rs.randint(0, 65536, (H, W)).astype(np.uint16), rs.randint(0, 65536, (H // 2, W // 2, 2)).astype(np.uint16)]
    if layout in ("i420", "yv12"):
        return [r8(H, W), r8(H // 2, W // 2), r8(H // 2, W // 2)]
    if layout in ("yuyv", "uyvy"):
        return [r8(H, W, 2)]
    raise ValueError(layout)
