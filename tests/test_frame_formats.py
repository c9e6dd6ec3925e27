"""CPU: frames in other pixel formats (vt_image, include/vittrack.h) -- the numpy oracle of rgb(d) against hand-worked values, the
descriptor's layout against the C header, ImageTable.check's poison rules, the packing of host planes and the Image constructors."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from pixel_oracle import nv_to_rgb, rgb_of, yuv_to_rgb


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def test_limited_range_endpoints():
    # Y = 16 / 235 with neutral chroma: black and white
    assert yuv_to_rgb(16, 128, 128).tolist() == [0, 0, 0]
    assert yuv_to_rgb(235, 128, 128).tolist() == [255, 255, 255]
    # below 16 the luma term is 0 (max(Y - 16, 0)), not negative
    assert yuv_to_rgb(0, 128, 128).tolist() == [0, 0, 0]


# (Y, U, V) -> (R, G, B), worked by hand from the formula (yy = max(Y - 16, 0) * 1220542, 2^20 = 1048576):
#   (81, 90, 240): yy = 79335230, u = -38, v = 112
#       R = (79335230 + 187435024 + 524288) >> 20 = 267294542 >> 20 = 254
#       G = (79335230 - 95479104 + 15579734 + 524288) >> 20 = -39852 >> 20 = -1 -> 0          (negative before the shift)
#       B = (79335230 - 80408988 + 524288) >> 20 = -549470 >> 20 = -1 -> 0
#   (255, 255, 255): yy = 291709538, u = v = 127
#       R = 504771755 >> 20 = 481 -> 255;  G = (291709538 - 108266484 - 52069111 + 524288) >> 20 = 131898231 >> 20 = 125;  B -> 255
#   (0, 0, 0): yy = 0, u = v = -128
#       R = -213687168 >> 20 -> 0;  G = (109118976 + 52479104 + 524288) >> 20 = 162122368 >> 20 = 154;  B -> 0
#   (16, 128, 127): R = -1149239 >> 20 = -2 -> 0;  G = 1376780 >> 20 = 1;  B = 524288 >> 20 = 0
HAND = [((81, 90, 240), (254, 0, 0)), ((255, 255, 255), (255, 125, 255)), ((0, 0, 0), (0, 154, 0)), ((16, 128, 127), (0, 1, 0))]


@pytest.mark.parametrize("yuv,rgb", HAND)
def test_hand_worked_values(yuv, rgb):
    assert tuple(yuv_to_rgb(*yuv).tolist()) == rgb


def test_clamping_at_both_ends():
    Y, U, V = np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing="ij")
    out = yuv_to_rgb(Y, U, V)
    yy = np.maximum(Y - 16, 0) * 1220542
    raw_r = (yy + 1673527 * (V - 128) + (1 << 19)) >> 20
    assert (raw_r < 0).any() and (raw_r > 255).any()
    assert np.array_equal(out[..., 0], np.clip(raw_r, 0, 255))


def test_nv12_equals_nv21_with_swapped_pairs():
    rs = np.random.RandomState(0)
    y = rs.randint(0, 256, (6, 8)).astype(np.uint8)
    uv = rs.randint(0, 256, (3, 4, 2)).astype(np.uint8)
    a = nv_to_rgb(y, uv)
    assert np.array_equal(a, nv_to_rgb(y, uv[..., ::-1], nv21=True))
    # a 2 x 2 block shares its chroma pair: pixel (3, 5) uses pair (1, 2)
    assert a[3, 5].tolist() == yuv_to_rgb(y[3, 5], uv[1, 2, 0], uv[1, 2, 1]).tolist()


def test_packed_formats():
    rs = np.random.RandomState(1)
    f = rs.randint(0, 256, (5, 7, 4)).astype(np.uint8)
    assert np.array_equal(rgb_of("rgba", [f]), f[..., :3])
    assert np.array_equal(rgb_of("bgra", [f]), f[..., [2, 1, 0]])
    assert np.array_equal(rgb_of("bgr", [f[..., :3]]), f[..., [2, 1, 0]])


# ---- the descriptor ------------------------------------------------------------------------------------------------------------
_CTYPES = {"const uint8_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


def _header_struct(name):
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const uint8_t\*|int64_t|int32_t)\s+(.*)", decl)
        for n in m.group(2).split(","):
            fields.append((n.strip().lstrip("*"), _CTYPES[m.group(1)]))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def test_image_dtype_matches_the_c_struct():
    from vittracker_amd.native import IMAGE_DTYPE
    S = _header_struct("vt_image")
    assert ctypes.sizeof(S) == IMAGE_DTYPE.itemsize == 48
    assert [f for f, _ in S._fields_] == list(IMAGE_DTYPE.names)
    for f, _ in S._fields_:
        assert getattr(S, f).offset == IMAGE_DTYPE.fields[f][1], f
        assert getattr(S, f).size == IMAGE_DTYPE.fields[f][0].itemsize, f


def test_format_codes_match_the_header():
    from vittracker_amd import native
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    codes = dict((k, int(v)) for k, v in re.findall(r"VT_PIX_(\w+) = (\d+)", src))
    assert codes == {"RGB": native.PIX_RGB, "BGR": native.PIX_BGR, "RGBA": native.PIX_RGBA, "BGRA": native.PIX_BGRA,
                     "NV12": native.PIX_NV12, "NV21": native.PIX_NV21}


# ---- ImageTable.check: the device's poison rules on the host -------------------------------------------------------------------
P0, P1 = 0x10000, 0x20000


def _ok(fmt, **kw):
    from vittracker_amd.native import ImageTable
    a = dict(fmt=fmt, ptr0=P0, ptr1=P1, H=40, W=60, pitch0=0, pitch1=0, reserved=0)
    a.update(kw)
    return ImageTable.check(**a)


@pytest.mark.parametrize("fmt", range(6))
def test_check_accepts_good_descriptors(fmt):
    from vittracker_amd import native
    p0, p1 = _ok(fmt)
    row = {0: 180, 1: 180, 2: 240, 3: 240, 4: 60, 5: 60}[fmt]
    assert p0 == row
    if fmt >= native.PIX_NV12:
        assert p1 == 60
    assert _ok(fmt, pitch0=row + 36)[0] == row + 36
    if fmt < native.PIX_NV12:
        _ok(fmt, ptr1=0, pitch1=-5)          # plane 1 is not needed: anything goes


POISON = [
    ("unknown format", dict(fmt=6)), ("negative format", dict(fmt=-1)), ("reserved", dict(fmt=0, reserved=1)),
    ("null plane0", dict(fmt=0, ptr0=0)), ("misaligned plane0", dict(fmt=2, ptr0=P0 + 2)),
    ("null plane1", dict(fmt=4, ptr1=0)), ("misaligned plane1", dict(fmt=5, ptr1=P1 + 1)),
    ("short pitch0", dict(fmt=1, pitch0=179)), ("short pitch0 rgba", dict(fmt=3, pitch0=239)), ("short pitch0 nv", dict(fmt=4, pitch0=59)),
    ("short pitch1", dict(fmt=4, pitch1=59)), ("odd H", dict(fmt=4, H=41)), ("odd W", dict(fmt=5, W=61)), ("H < 1", dict(fmt=0, H=0)),
    ("W < 1", dict(fmt=4, W=0)), ("32-bit extent", dict(fmt=2, H=70000, W=20000)), ("32-bit chroma", dict(fmt=4, pitch1=1 << 31)),
]


@pytest.mark.parametrize("what,kw", POISON, ids=[p[0] for p in POISON])
def test_check_rejects_every_poison_case(what, kw):
    from vittracker_amd.native import VtError
    with pytest.raises(VtError):
        _ok(**kw)


def test_check_bounds_each_plane_by_its_buffer():
    from vittracker_amd.native import ImageTable, VtError
    ImageTable.check(4, P0, P1, 40, 60, 64, 0, 0, nbytes0=64 * 39 + 60, nbytes1=60 * 19 + 60)
    with pytest.raises(VtError):
        ImageTable.check(4, P0, P1, 40, 60, 64, 0, 0, nbytes0=64 * 39 + 59)
    with pytest.raises(VtError):
        ImageTable.check(4, P0, P1, 40, 60, 0, 0, 0, nbytes1=60 * 19 + 59)


# ---- packing host planes -------------------------------------------------------------------------------------------------------
def test_host_planes_are_packed_disjoint_and_aligned():
    from vittracker_amd.native import Image, pack_image_offsets
    rs = np.random.RandomState(2)
    ims = [Image.nv12(rs.randint(0, 256, (6, 10)).astype(np.uint8), rs.randint(0, 256, (3, 5, 2)).astype(np.uint8)),
           Image.bgr(rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)),
           Image.rgba(rs.randint(0, 256, (3, 3, 4)).astype(np.uint8)),
           Image.nv21(rs.randint(0, 256, (2, 2)).astype(np.uint8), rs.randint(0, 256, (1, 1, 2)).astype(np.uint8))]
    offs, end = pack_image_offsets(ims, start=4 * 48)
    spans = []
    for im, po in zip(ims, offs):
        assert len(po) == len(im.planes)
        for o, (rows, rb) in zip(po, im.plane_rows()):
            assert o % 256 == 0 and o >= 4 * 48
            spans.append((o, o + rows * rb))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert end == spans[-1][1]


# ---- Image constructors --------------------------------------------------------------------------------------------------------
def test_constructors_take_good_planes():
    from vittracker_amd import native
    from vittracker_amd.native import Image
    f3 = np.zeros((4, 6, 3), np.uint8)
    f4 = np.zeros((4, 6, 4), np.uint8)
    assert Image.rgb(f3).format == native.PIX_RGB and Image.bgr(f3).format == native.PIX_BGR
    assert Image.rgba(f4).format == native.PIX_RGBA and Image.bgra(f4).pitches == (24,)
    wide = np.zeros((4, 9, 3), np.uint8)[:, 2:8]          # a window of a wider frame: pitch 27
    assert Image.bgr(wide).pitches == (27,) and Image.bgr(wide).shape == (4, 6, 3)
    nv = Image.nv12(np.zeros((4, 6), np.uint8), np.zeros((2, 3, 2), np.uint8))
    assert (nv.H, nv.W, nv.pitches, nv.format) == (4, 6, (6, 6), native.PIX_NV12)
    assert Image.nv21(np.zeros((4, 8), np.uint8)[:, :6], np.zeros((2, 4, 2), np.uint8)[:, :3]).pitches == (8, 8)


BAD = [
    ("rgb with 4 channels", lambda I: I.rgb(np.zeros((4, 6, 4), np.uint8))),
    ("rgba with 3 channels", lambda I: I.rgba(np.zeros((4, 6, 3), np.uint8))),
    ("rgb 2-d", lambda I: I.rgb(np.zeros((4, 6), np.uint8))),
    ("float", lambda I: I.bgr(np.zeros((4, 6, 3), np.float32))),
    ("int16", lambda I: I.nv12(np.zeros((4, 6), np.int16), np.zeros((2, 3, 2), np.uint8))),
    ("strided pixels", lambda I: I.rgb(np.zeros((4, 12, 3), np.uint8)[:, ::2])),
    ("strided channels", lambda I: I.bgra(np.zeros((4, 6, 8), np.uint8)[:, :, ::2])),
    ("odd H", lambda I: I.nv12(np.zeros((5, 6), np.uint8), np.zeros((2, 3, 2), np.uint8))),
    ("odd W", lambda I: I.nv21(np.zeros((4, 7), np.uint8), np.zeros((2, 3, 2), np.uint8))),
    ("chroma shape", lambda I: I.nv12(np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8))),
    ("chroma size", lambda I: I.nv12(np.zeros((4, 6), np.uint8), np.zeros((4, 3, 2), np.uint8))),
    ("strided luma", lambda I: I.nv12(np.zeros((4, 12), np.uint8)[:, ::2], np.zeros((2, 3, 2), np.uint8))),
    ("strided chroma", lambda I: I.nv12(np.zeros((4, 6), np.uint8), np.zeros((2, 6, 2), np.uint8)[:, ::2])),
    ("not an array", lambda I: I.rgb([[[0, 0, 0]]])),
]


@pytest.mark.parametrize("what,make", BAD, ids=[b[0] for b in BAD])
def test_constructors_reject_bad_planes(what, make):
    from vittracker_amd.native import Image, VtError
    with pytest.raises(VtError):
        make(Image)
