"""numpy oracle of rgb(d), the RGB image a vt_image descriptor denotes (include/vittrack.h), written from the formula alone: no product
code.  NV12 / NV21: BT.601 limited range in OpenCV's fixed point (cv.cvtColor(f, cv.COLOR_YUV2RGB_NV12 / _NV21)), each 2 x 2 block
sharing one chroma pair."""
import numpy as np

FORMATS = ("rgb", "bgr", "rgba", "bgra", "nv12", "nv21")


def yuv_to_rgb(Y, U, V):
    """int arrays of equal shape -> (..., 3) uint8.  int64 throughout; numpy's >> on a negative value is arithmetic (floor)."""
    Y, U, V = (np.asarray(a, dtype=np.int64) for a in (Y, U, V))
    yy = np.maximum(Y - 16, 0) * 1220542
    u, v = U - 128, V - 128
    R = (yy + 1673527 * v + (1 << 19)) >> 20
    G = (yy - 852492 * v - 409993 * u + (1 << 19)) >> 20
    B = (yy + 2116026 * u + (1 << 19)) >> 20
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def nv_to_rgb(y, c, nv21=False):
    """y (H, W) luma, c (H/2, W/2, 2) chroma pairs ((U, V); (V, U) for NV21) -> (H, W, 3) uint8."""
    y = np.asarray(y)
    c = np.asarray(c)
    U, V = (c[..., 1], c[..., 0]) if nv21 else (c[..., 0], c[..., 1])
    up = lambda a: np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)      # noqa: E731  no chroma interpolation
    return yuv_to_rgb(y, up(U), up(V))


def rgb_of(fmt, planes):
    """rgb(d) of a format name and its planes (numpy)."""
    if fmt == "rgb":
        return np.ascontiguousarray(planes[0][..., :3])
    if fmt == "bgr":
        return np.ascontiguousarray(planes[0][..., 2::-1])
    if fmt == "rgba":
        return np.ascontiguousarray(planes[0][..., :3])
    if fmt == "bgra":
        return np.ascontiguousarray(planes[0][..., 2::-1])
    if fmt in ("nv12", "nv21"):
        return nv_to_rgb(planes[0], planes[1], nv21=fmt == "nv21")
    raise ValueError(fmt)


def random_planes(rs, fmt, H, W):
    """Random planes of an H x W image in `fmt` (numpy, tight)."""
    if fmt in ("rgb", "bgr"):
        return [rs.randint(0, 256, (H, W, 3)).astype(np.uint8)]
    if fmt in ("rgba", "bgra"):
        return [rs.randint(0, 256, (H, W, 4)).astype(np.uint8)]
    return [rs.randint(0, 256, (H, W)).astype(np.uint8), rs.randint(0, 256, (H // 2, W // 2, 2)).astype(np.uint8)]
