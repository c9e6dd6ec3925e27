"""numpy oracle of rgb(d) for the wide layouts of vt_image (include/vittrack.h): YV16 / YV24, NV16 / NV24, P210 / P410 and the planar
layouts in LSB-aligned 16-bit words (I010 ... I416, GRAY10 / GRAY12 / GRAY16).  Written from the header's rules alone, int64 throughout:
no product code.  The 8-bit sample of a 16-bit word is s8 = min(v >> (depth - 8), 255) (P210 / P410: the high byte, i.e. depth 16); the
colour arithmetic and its four coefficient rows are tests/pixel_oracle_yuv.py's; chroma is never interpolated."""
import numpy as np

from pixel_oracle_yuv import COLOURS, yuv_to_rgb

SUBS = ("420", "422", "444", "gray")
DEPTHS = (10, 12, 16)
_STEM = {"420": "i0", "422": "i2", "444": "i4", "gray": "gray"}
#: layout name -> (code, sub, container: "v3" three byte planes V first | "sp" luma + pairs | "p3" three planes | "g" luma only, depth)
LAYOUTS = {"yv16": (21, "422", "v3", 8), "yv24": (22, "444", "v3", 8), "nv16": (23, "422", "sp", 8), "nv24": (24, "444", "sp", 8),
           "p210": (25, "422", "sp", 16), "p410": (26, "444", "sp", 16)}
for _si, _s in enumerate(SUBS):
    for _di, _d in enumerate(DEPTHS):
        LAYOUTS[_STEM[_s] + str(_d)] = (32 | _si << 2 | _di, _s, "g" if _s == "gray" else "p3", _d)
LAYOUT_CODE = {k: v[0] for k, v in LAYOUTS.items()}
WIDE_LAYOUTS = tuple(LAYOUTS)
WIDE_YUV = tuple(k for k, v in LAYOUTS.items() if v[1] != "gray")
WIDE_GRAY = tuple(k for k, v in LAYOUTS.items() if v[1] == "gray")
#: fetched as aligned 16-bit words: even addresses and pitches
WIDE_LSB = tuple(k for k, v in LAYOUTS.items() if v[3] in (10, 12))
#: every legal (layout, matrix, range): the four colour rows on the YUV layouts, none on the grey ones
COMBOS = [(lay, m, r) for lay in WIDE_YUV for (m, r) in COLOURS] + [(lay, "bt601", "limited") for lay in WIDE_GRAY]
#: codes that stay unassigned
UNASSIGNED = (6, 7, 14, 15, 20, 27, 28, 29, 30, 31, 35, 39, 43, 47, 48)


def format_word(layout, matrix="bt601", rng="limited"):
    return LAYOUT_CODE[layout] | (("bt601", "bt709").index(matrix) << 8) | (("limited", "full").index(rng) << 12)


def sub_of(layout):
    return LAYOUTS[layout][1]


def depth_of(layout):
    """Bits of a sample: 8 (bytes), 10, 12 or 16 (P210 / P410: MSB-aligned words, read as depth 16)."""
    return LAYOUTS[layout][3]


def legal_size(layout, H, W):
    s = sub_of(layout)
    return (H % 2 == 0 and W % 2 == 0) if s == "420" else (W % 2 == 0 if s == "422" else True)


def fit_size(layout, H, W):
    """(H, W) with the odd dimension the layout's subsampling forbids made even (one less)."""
    s = sub_of(layout)
    return (H - H % 2 if s == "420" else H), (W - W % 2 if s in ("420", "422") else W)


def chroma_shape(layout, H, W):
    s = sub_of(layout)
    return (H // 2 if s == "420" else H), (W if s == "444" else W // 2)


def row_bytes(layout, W):
    """Bytes of a row of plane 0 and of plane 1 (0: none)."""
    _, s, kind, d = LAYOUTS[layout]
    b = 1 if d == 8 else 2
    if kind == "g":
        return b * W, 0
    return b * W, b * chroma_shape(layout, 2, W)[1] * (2 if kind == "sp" else 1)


def plane1_rows(layout, H):
    """Rows of plane 1: a plane of pairs has H; three-plane layouts hold both chroma planes back to back."""
    kind = LAYOUTS[layout][2]
    return H if kind == "sp" else 2 * chroma_shape(layout, H, 2)[0]


def extents(layout, H, W, pitch0=0, pitch1=0):
    """Bytes of plane 0 and plane 1: pitch (rows - 1) + row bytes."""
    r0, r1 = row_bytes(layout, W)
    p0, p1 = pitch0 or r0, pitch1 or r1
    return p0 * (H - 1) + r0, (p1 * (plane1_rows(layout, H) - 1) + r1 if r1 else 0)


def s8(words, depth):
    """The 8-bit sample of a word: min(v >> (depth - 8), 255); a byte is itself."""
    v = np.asarray(words).astype(np.int64) & (0xffff if depth > 8 else 0xff)
    return np.minimum(v >> (depth - 8), 255)


def words_of(samples, depth, low=None):
    """Words whose 8-bit sample is `samples`: s8 << (depth - 8) | low, low the junk below the sample (None: zero)."""
    v = np.asarray(samples).astype(np.int64) << (depth - 8)
    if low is not None:
        v = v | (np.asarray(low).astype(np.int64) & ((1 << (depth - 8)) - 1))
    return v.astype(np.uint16 if depth > 8 else np.uint8)


def planes_of_yuv(layout, Y, U, V, rs=None):
    """The planes of `layout`, in the shapes the Image constructors take, whose 8-bit samples are Y (H, W) and U, V (chroma_shape);
    rs: a RandomState that fills the bits below each sample with junk (None: zeros)."""
    _, s, kind, d = LAYOUTS[layout]
    low = (lambda a: rs.randint(0, 65536, np.shape(a))) if rs is not None else (lambda a: None)
    w = lambda a: words_of(a, d, low(a))      # noqa: E731
    if kind == "g":
        return [w(Y)]
    assert np.shape(U) == np.shape(V) == chroma_shape(layout, *np.shape(Y)), (layout, np.shape(Y), np.shape(U))
    if kind == "v3":
        return [w(Y), w(V), w(U)]
    if kind == "sp":
        return [w(Y), np.stack([w(U), w(V)], axis=-1)]
    return [w(Y), w(U), w(V)]


def samples_of(layout, planes):
    """(Y, U, V) 8-bit samples, int64, of planes as planes_of_yuv lays them out (grey: U = V = None)."""
    _, s, kind, d = LAYOUTS[layout]
    if kind == "g":
        return s8(planes[0], d), None, None
    if kind == "v3":
        return s8(planes[0], d), s8(planes[2], d), s8(planes[1], d)
    if kind == "sp":
        c = s8(planes[1], d)
        return s8(planes[0], d), c[..., 0], c[..., 1]
    return s8(planes[0], d), s8(planes[1], d), s8(planes[2], d)


def rgb_of(layout, planes, matrix="bt601", rng="limited"):
    """rgb(d) of a layout name and its planes."""
    Y, U, V = samples_of(layout, planes)
    if U is None:
        return np.ascontiguousarray(np.repeat(Y[..., None], 3, axis=2)).astype(np.uint8)
    H, W = Y.shape
    s = sub_of(layout)
    yi = np.arange(H) >> (1 if s == "420" else 0)
    xi = np.arange(W) >> (0 if s == "444" else 1)
    return yuv_to_rgb(Y, U[yi][:, xi], V[yi][:, xi], matrix, rng)


def yuv_of_rgb(layout, rgb, matrix="bt601", rng="limited"):
    """8-bit (Y, U, V) of an RGB image for `layout`: the fp64 forward transform, rounded; chroma taken from the top-left pixel of each
    block (what an uninterpolated decode hands back to every pixel of it)."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    r, g, b = (np.asarray(rgb)[..., i].astype(np.float64) for i in range(3))
    y = kr * r + (1 - kr - kb) * g + kb * b
    u, v = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    ls, cs, yo = (219.0 / 255.0, 224.0 / 255.0, 16.0) if rng == "limited" else (1.0, 1.0, 0.0)
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)      # noqa: E731
    Y, U, V = q(y * ls + yo), q(u * cs + 128.0), q(v * cs + 128.0)
    s = sub_of(layout)
    sy, sx = (2 if s == "420" else 1), (1 if s in ("444", "gray") else 2)
    return Y, U[::sy, ::sx], V[::sy, ::sx]


def planes_of_rgb(layout, rgb, matrix="bt601", rng="limited", rs=None):
    Y, U, V = yuv_of_rgb(layout, rgb, matrix, rng)
    return planes_of_yuv(layout, Y, U, V, rs)


def random_planes(rs, layout, H, W):
    """Random planes of an H x W image: every bit below the sample random; of the 10- / 12-bit words about one in sixteen lies above
    the depth's range (it saturates), the others spread their samples over 0 ... 255."""
    d = depth_of(layout)
    ch, cw = chroma_shape(layout, H, W)

    def full(*sh):
        if d == 8:
            return rs.randint(0, 256, sh).astype(np.uint8)
        a = rs.randint(0, 1 << d, sh)
        over = rs.randint(0, 16, sh) == 0
        return np.where(over, rs.randint(0, 65536, sh), a).astype(np.uint16)
    kind = LAYOUTS[layout][2]
    if kind == "g":
        return [full(H, W)]
    if kind == "sp":
        return [full(H, W), full(ch, cw, 2)]
    return [full(H, W), full(ch, cw), full(ch, cw)]


def in_range_planes(rs, layout, H, W):
    """As random_planes with every word inside the depth's range, so that the samples spread over 0 ... 255 and do not saturate."""
    d = depth_of(layout)
    return [(p & ((1 << d) - 1)).astype(p.dtype) if d > 8 else p for p in random_planes(rs, layout, H, W)]
