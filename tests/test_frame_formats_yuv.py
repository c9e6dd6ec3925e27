"""CPU: the layouts and colour rows added to vt_image (I420 / YV12, YUYV / UYVY, P010, GRAY8; BT.709 and full range for every YUV
layout) -- the new numpy oracle against the old one and against the fp64 formula, the format word, ImageTable.check's accept / reject
matrix, the Image constructors and the packing of host planes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import pixel_oracle
import pixel_oracle_yuv as oy

P0, P1 = 0x10000, 0x20000
LAYOUTS = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3, "nv12": 4, "nv21": 5, "i420": 8, "yv12": 9, "yuyv": 10, "uyvy": 11, "p010": 12, "gray8": 13}
YUV = ("nv12", "nv21", "i420", "yv12", "yuyv", "uyvy", "p010")


@pytest.fixture(scope="module")
def all_triples():
    Y, U, V = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    return Y.ravel(), U.ravel(), V.ravel()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def test_601_limited_row_is_the_old_oracle(all_triples):
    Y, U, V = all_triples
    assert np.array_equal(oy.yuv_to_rgb(Y, U, V, "bt601", "limited"), pixel_oracle.yuv_to_rgb(Y, U, V))


@pytest.mark.parametrize("matrix,rng", [("bt601", "full"), ("bt709", "limited"), ("bt709", "full")])
def test_fixed_point_against_fp64(all_triples, matrix, rng):
    """Coefficients are round(x 2^20): before clamping each channel is within 0.51 of the fp64 formula (measured 0.5000 / 0.5002 /
    0.5000), the pre-shift value fits int32, and the clamped integer is within 1 of round(clip(truth))."""
    Y, U, V = all_triples
    fx = oy.fixed_point(Y, U, V, matrix, rng)
    assert int(np.abs(fx).max()) < 2 ** 31
    truth = oy.truth_fp64(Y, U, V, matrix, rng)
    err = np.abs((fx >> 20).astype(np.float64) - truth).max(axis=0)
    print(matrix, rng, "max |fixed - fp64| per channel:", err, "max pre-shift:", int(np.abs(fx).max()))
    assert (err <= 0.51).all(), err
    got = np.clip(fx >> 20, 0, 255)
    want = np.rint(np.clip(truth, 0.0, 255.0)).astype(np.int64)
    assert int(np.abs(got - want).max()) <= 1


def test_coefficients_are_the_rounded_rationals():
    for (matrix, rng), row in oy.COEF.items():
        if (matrix, rng) == ("bt601", "limited"):
            continue                               # OpenCV's literals, kept as they are
        kr, kb = oy.KR_KB[matrix]
        kg = 1 - kr - kb
        ls, cs = (255 / 219, 255 / 224) if rng == "limited" else (1.0, 1.0)
        want = [ls, cs * 2 * (1 - kr), cs * 2 * (1 - kr) * kr / kg, cs * 2 * (1 - kb) * kb / kg, cs * 2 * (1 - kb)]
        assert list(row) == [int(round(x * 2 ** 20)) for x in want], (matrix, rng)


def test_full_range_endpoints_and_gray():
    assert oy.yuv_to_rgb(0, 128, 128, "bt709", "full").tolist() == [0, 0, 0]
    assert oy.yuv_to_rgb(255, 128, 128, "bt601", "full").tolist() == [255, 255, 255]
    assert oy.yuv_to_rgb(16, 128, 128, "bt709", "limited").tolist() == [0, 0, 0]
    assert oy.yuv_to_rgb(235, 128, 128, "bt709", "limited").tolist() == [255, 255, 255]
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(oy.rgb_of("gray", [g]), np.stack([g, g, g], axis=-1))


def test_layouts_share_chroma_as_described():
    rs = np.random.RandomState(0)
    H, W = 4, 6
    y, u, v = oy.random_planes(rs, "i420", H, W)
    ref = oy.rgb_of("i420", [y, u, v], "bt709", "full")
    assert ref[3, 5].tolist() == oy.yuv_to_rgb(y[3, 5], u[1, 2], v[1, 2], "bt709", "full").tolist()
    assert np.array_equal(oy.rgb_of("yv12", [y, v, u], "bt709", "full"), ref)
    assert np.array_equal(oy.rgb_of("nv12", [y, np.stack([u, v], axis=-1)], "bt709", "full"), ref)
    # P010: the high byte is the sample, the low byte is ignored
    lo = rs.randint(0, 256, (H, W)).astype(np.uint16)
    y16 = (y.astype(np.uint16) << 8) | lo
    c16 = (np.stack([u, v], axis=-1).astype(np.uint16) << 8) | 0x00c0
    assert np.array_equal(oy.rgb_of("p010", [y16, c16], "bt709", "full"), ref)
    # packed 4:2:2: chroma of each pair of pixels, every row its own
    p = oy.random_planes(rs, "yuyv", H, W)[0]
    a = oy.rgb_of("yuyv", [p], "bt601", "full")
    assert a[2, 3].tolist() == oy.yuv_to_rgb(p[2, 3, 0], p[2, 2, 1], p[2, 3, 1], "bt601", "full").tolist()
    q = p[..., ::-1].copy()
    assert np.array_equal(oy.rgb_of("uyvy", [q], "bt601", "full"), a)


# ---- the format word -----------------------------------------------------------------------------------------------------------
def test_format_word_fields_and_header():
    from vittracker_amd import native
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    defs = dict((k, int(v, 0)) for k, v in re.findall(r"#define VT_PIX_(\w+) (0x[0-9a-fA-F]+|\d+)\b", src))
    assert {k: defs[k] for k in ("I420", "YV12", "YUYV", "UYVY", "P010", "GRAY8")} == {
        "I420": native.PIX_I420, "YV12": native.PIX_YV12, "YUYV": native.PIX_YUYV, "UYVY": native.PIX_UYVY, "P010": native.PIX_P010,
        "GRAY8": native.PIX_GRAY8} == {"I420": 8, "YV12": 9, "YUYV": 10, "UYVY": 11, "P010": 12, "GRAY8": 13}
    assert (defs["BT601"], defs["BT709"], defs["LIMITED"], defs["FULL"]) == (0, 1 << 8, 0, 1 << 12)
    assert native.PIX_NAMES[:6] == ("rgb", "bgr", "rgba", "bgra", "nv12", "nv21") and native.IMAGE_DTYPE.itemsize == 48
    for name, lay in LAYOUTS.items():
        for mi, m in enumerate(("bt601", "bt709")):
            for ri, r in enumerate(("limited", "full")):
                w = native.pix_format(lay, m, r)
                assert w == lay | (mi << 8) | (ri << 12) and native.pix_fields(w) == (lay, mi, ri, 0)
                if name != "gray8":
                    assert w == oy.format_word(name, m, r)
    assert native.pix_format(native.PIX_NV12) == native.PIX_NV12        # every value legal before means what it meant
    with pytest.raises(native.VtError):
        native.pix_format(native.PIX_NV12, matrix="bt2020")
    with pytest.raises(native.VtError):
        native.pix_format(native.PIX_NV12, range="video")


def test_sizeof_vt_image_is_still_48():
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    body = re.search(r"typedef struct vt_image \{(.*?)\} vt_image;", src, re.S).group(1)
    ct = {"const uint8_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const uint8_t\*|int64_t|int32_t)\s+(.*)", decl)
        fields += [(n.strip().lstrip("*"), ct[m.group(1)]) for n in m.group(2).split(",")]
    S = type("vt_image", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(S) == 48 and [f for f, _ in fields][-2:] == ["format", "reserved"]


# ---- ImageTable.check ----------------------------------------------------------------------------------------------------------
def _ok(fmt, **kw):
    from vittracker_amd.native import ImageTable
    a = dict(fmt=fmt, ptr0=P0, ptr1=P1, H=40, W=60, pitch0=0, pitch1=0, reserved=0)
    a.update(kw)
    return ImageTable.check(**a)


#: layout -> (row bytes of plane 0, row bytes of plane 1) at W = 60
ROWS = {"rgb": (180, 0), "bgr": (180, 0), "rgba": (240, 0), "bgra": (240, 0), "nv12": (60, 60), "nv21": (60, 60), "i420": (60, 30),
        "yv12": (60, 30), "yuyv": (120, 0), "uyvy": (120, 0), "p010": (120, 120), "gray8": (60, 0)}
LEGAL = [(n, m, r) for n in LAYOUTS for m in (0, 1) for r in (0, 1) if n in YUV or (m, r) == (0, 0)]


@pytest.mark.parametrize("name,m,r", LEGAL, ids=["%s-%d%d" % t for t in LEGAL])
def test_check_accepts_every_legal_word(name, m, r):
    p0, p1 = _ok(LAYOUTS[name] | (m << 8) | (r << 12))
    assert p0 == ROWS[name][0]
    if ROWS[name][1]:
        assert p1 == ROWS[name][1]
    assert _ok(LAYOUTS[name] | (m << 8) | (r << 12), pitch0=p0 + 36)[0] == p0 + 36


POISON = [
    ("layout 6", dict(fmt=6)), ("layout 7", dict(fmt=7)), ("layout 14", dict(fmt=14)), ("layout 6 with colour", dict(fmt=6 | 1 << 8)),
    ("bit 16", dict(fmt=4 | 1 << 16)), ("bit 31", dict(fmt=8 | 1 << 31)), ("bit 20 on rgb", dict(fmt=1 << 20)),
    ("matrix 2", dict(fmt=4 | 2 << 8)), ("range 2", dict(fmt=12 | 2 << 12)),
    ("matrix on rgb", dict(fmt=0 | 1 << 8)), ("range on bgra", dict(fmt=3 | 1 << 12)), ("matrix on gray8", dict(fmt=13 | 1 << 8)),
    ("range on gray8", dict(fmt=13 | 1 << 12)),
    ("odd W yuyv", dict(fmt=10, W=61)), ("odd W uyvy", dict(fmt=11 | 1 << 8, W=59)), ("odd H i420", dict(fmt=8, H=41)),
    ("odd W yv12", dict(fmt=9, W=61)), ("odd H p010", dict(fmt=12, H=39)),
    ("short pitch1 i420", dict(fmt=8, pitch1=29)), ("short pitch1 p010", dict(fmt=12, pitch1=119)),
    ("short pitch0 p010", dict(fmt=12, pitch0=119)), ("short pitch0 yuyv", dict(fmt=10, pitch0=119)), ("short pitch0 gray8", dict(fmt=13, pitch0=59)),
    ("null plane1 i420", dict(fmt=8, ptr1=0)), ("misaligned plane1 p010", dict(fmt=12, ptr1=P1 + 2)), ("reserved", dict(fmt=13, reserved=1)),
    ("32-bit chroma i420", dict(fmt=8, pitch1=1 << 31)),
]


@pytest.mark.parametrize("what,kw", POISON, ids=[p[0] for p in POISON])
def test_check_rejects_every_poison_case(what, kw):
    from vittracker_amd.native import VtError
    with pytest.raises(VtError):
        _ok(**kw)


def test_check_lets_one_plane_layouts_ignore_plane1_and_yuyv_take_odd_h():
    _ok(13, ptr1=0, pitch1=-5)
    _ok(10, ptr1=0, H=41)
    _ok(11 | 1 << 8 | 1 << 12, H=1, W=2)


def test_check_bounds_the_second_chroma_plane_by_the_buffer():
    """I420's plane-1 extent covers BOTH chroma planes: pitch1 (H - 1) + W / 2 bytes; P010's rows are 2 W bytes."""
    from vittracker_amd.native import ImageTable, VtError
    ImageTable.check(8, P0, P1, 40, 60, 0, 32, 0, nbytes0=2400, nbytes1=32 * 39 + 30)
    with pytest.raises(VtError):
        ImageTable.check(8, P0, P1, 40, 60, 0, 32, 0, nbytes1=32 * 39 + 29)
    with pytest.raises(VtError):
        ImageTable.check(8, P0, P1, 40, 60, 0, 0, 0, nbytes1=30 * 20)             # room for the first chroma plane only
    ImageTable.check(12, P0, P1, 40, 60, 0, 0, 0, nbytes0=120 * 40, nbytes1=120 * 20)
    with pytest.raises(VtError):
        ImageTable.check(12, P0, P1, 40, 60, 0, 0, 0, nbytes1=120 * 20 - 1)
    with pytest.raises(VtError):
        ImageTable.check(12, P0, P1, 40, 60, 0, 0, 0, nbytes0=60 * 40)            # a luma plane of W-byte rows is half of it


# ---- constructors --------------------------------------------------------------------------------------------------------------
def test_constructors_take_good_planes():
    from vittracker_amd import native
    from vittracker_amd.native import Image
    z = lambda *s: np.zeros(s, np.uint8)      # noqa: E731
    im = Image.i420(z(4, 6), z(2, 3), z(2, 3), matrix="bt709")
    assert (im.H, im.W, im.pitches, im.format) == (4, 6, (6, 3), native.PIX_I420 | 1 << 8) and im.plane_rows() == [(4, 6), (4, 3)]
    assert Image.yv12(z(4, 6), z(2, 3), z(2, 3), range="full").format == native.PIX_YV12 | 1 << 12
    b = Image.i420_buffer(z(6, 6), matrix="bt709", range="full")
    assert (b.H, b.W, b.pitches, b.format) == (4, 6, (6, 3), native.PIX_I420 | 1 << 8 | 1 << 12) and b.planes[1].shape == (4, 3)
    y = Image.yuyv(z(5, 6, 2))
    assert (y.H, y.W, y.pitches, y.format, y.plane_rows()) == (5, 6, (12,), native.PIX_YUYV, [(5, 12)])
    assert Image.uyvy(z(5, 8, 2)[:, :6], matrix="bt709").pitches == (16,)
    g = Image.gray(z(5, 7))
    assert (g.H, g.W, g.pitches, g.format, g.shape) == (5, 7, (7,), native.PIX_GRAY8, (5, 7, 3))
    assert Image.gray(z(5, 9)[:, 1:8]).pitches == (9,)
    p = Image.p010(np.zeros((4, 6), np.uint16), np.zeros((2, 3, 2), np.uint16), matrix="bt709")
    assert (p.H, p.W, p.pitches, p.format) == (4, 6, (12, 12), native.PIX_P010 | 1 << 8) and p.plane_rows() == [(4, 12), (2, 12)]
    assert p.planes[0].dtype == np.uint8 and p.planes[0].shape == (4, 12) and p.planes[1].shape == (2, 3, 4)
    q = Image.p010(z(4, 12), z(2, 3, 4))                                          # the uint8 views
    assert (q.H, q.W, q.pitches) == (4, 6, (12, 12))
    assert Image.p010(np.zeros((4, 8), np.uint16)[:, :6], np.zeros((2, 4, 2), np.int16)[:, :3]).pitches == (16, 16)
    assert Image.nv12(z(4, 6), z(2, 3, 2), matrix="bt709", range="full").format == native.PIX_NV12 | 1 << 8 | 1 << 12
    assert Image.nv21(z(4, 6), z(2, 3, 2)).format == native.PIX_NV21


def test_p010_takes_16_bit_tensors():
    import torch
    from vittracker_amd.native import Image
    p = Image.p010(torch.zeros(4, 6, dtype=torch.int16), torch.zeros(2, 3, 2, dtype=torch.int16))
    assert (p.H, p.W, p.pitches) == (4, 6, (12, 12)) and p.planes[0].dtype == torch.uint8
    if hasattr(torch, "uint16"):
        assert Image.p010(torch.zeros(4, 6, dtype=torch.uint16), torch.zeros(2, 3, 2, dtype=torch.uint16)).pitches == (12, 12)


def _z(*s):
    return np.zeros(s, np.uint8)


BAD = [
    ("i420 chroma shape", lambda I: I.i420(_z(4, 6), _z(2, 3, 1), _z(2, 3))),
    ("i420 chroma size", lambda I: I.i420(_z(4, 6), _z(2, 3), _z(4, 3))),
    ("i420 odd H", lambda I: I.i420(_z(5, 6), _z(2, 3), _z(2, 3))),
    ("i420 odd W", lambda I: I.yv12(_z(4, 7), _z(2, 3), _z(2, 3))),
    ("i420 strided luma", lambda I: I.i420(_z(4, 12)[:, ::2], _z(2, 3), _z(2, 3))),
    ("i420 strided chroma", lambda I: I.i420(_z(4, 6), _z(2, 6)[:, ::2], _z(2, 3))),
    ("i420 two chroma pitches", lambda I: I.i420(_z(4, 6), _z(2, 5)[:, :3], _z(2, 3))),
    ("i420 float", lambda I: I.i420(_z(4, 6), np.zeros((2, 3), np.float32), _z(2, 3))),
    ("i420 matrix", lambda I: I.i420(_z(4, 6), _z(2, 3), _z(2, 3), matrix="bt2020")),
    ("nv12 range", lambda I: I.nv12(_z(4, 6), _z(2, 3, 2), range="pc")),
    ("buffer rows", lambda I: I.i420_buffer(_z(7, 6))),
    ("buffer rows 2", lambda I: I.i420_buffer(_z(8, 6))),
    ("buffer odd W", lambda I: I.i420_buffer(_z(6, 7))),
    ("buffer pitch", lambda I: I.i420_buffer(_z(6, 8)[:, :6])),
    ("buffer 3-d", lambda I: I.i420_buffer(_z(6, 6, 1))),
    ("yuyv odd W", lambda I: I.yuyv(_z(4, 5, 2))),
    ("yuyv 3 bytes", lambda I: I.yuyv(_z(4, 6, 3))),
    ("uyvy 2-d", lambda I: I.uyvy(_z(4, 12))),
    ("yuyv strided pixels", lambda I: I.yuyv(_z(4, 12, 2)[:, ::2])),
    ("yuyv int16", lambda I: I.yuyv(np.zeros((4, 6, 2), np.int16))),
    ("gray 3-d", lambda I: I.gray(_z(4, 6, 1))),
    ("gray strided", lambda I: I.gray(_z(4, 12)[:, ::2])),
    ("gray float", lambda I: I.gray(np.zeros((4, 6), np.float32))),
    ("p010 32-bit", lambda I: I.p010(np.zeros((4, 6), np.uint32), np.zeros((2, 3, 2), np.uint16))),
    ("p010 big endian", lambda I: I.p010(np.zeros((4, 6), ">u2"), np.zeros((2, 3, 2), ">u2"))),
    ("p010 chroma shape", lambda I: I.p010(np.zeros((4, 6), np.uint16), np.zeros((2, 3), np.uint16))),
    ("p010 odd W", lambda I: I.p010(np.zeros((4, 7), np.uint16), np.zeros((2, 3, 2), np.uint16))),
    ("p010 odd byte width", lambda I: I.p010(_z(4, 13), _z(2, 3, 4))),
    ("p010 strided samples", lambda I: I.p010(np.zeros((4, 12), np.uint16)[:, ::2], np.zeros((2, 3, 2), np.uint16))),
    ("p010 short luma pitch", lambda I: I.p010(np.zeros((4, 6), np.uint16), np.zeros((2, 6, 2), np.uint16)[:, ::2])),
]


@pytest.mark.parametrize("what,make", BAD, ids=[b[0] for b in BAD])
def test_constructors_reject_bad_planes(what, make):
    from vittracker_amd.native import Image, VtError
    with pytest.raises(VtError):
        make(Image)


class _FakeDev:
    """A stand-in for a GPU plane: a uint8 tensor that says it is on the GPU, at an address of the test's choosing."""

    def __init__(self, t, ptr):
        self.t, self.ptr = t, ptr

    def make(self):
        import torch

        class T(torch.Tensor):
            @property
            def is_cuda(s):
                return True

            def data_ptr(s):
                return s._ptr
        r = self.t.as_subclass(T)
        r._ptr = self.ptr
        return r


def test_device_i420_needs_contiguous_chroma_planes():
    import torch
    from vittracker_amd.native import Image, VtError
    H, W = 4, 6
    y = _FakeDev(torch.zeros(H, W, dtype=torch.uint8), 0x1000).make()
    u = _FakeDev(torch.zeros(H // 2, W // 2, dtype=torch.uint8), 0x2000).make()
    good = _FakeDev(torch.zeros(H // 2, W // 2, dtype=torch.uint8), 0x2000 + 3 * 2).make()
    apart = _FakeDev(torch.zeros(H // 2, W // 2, dtype=torch.uint8), 0x3000).make()
    im = Image.i420(y, u, good)
    assert im.descriptor()[:4] == (0x1000, 0x2000, 6, 3)
    with pytest.raises(VtError, match="not contiguous"):
        Image.i420(y, u, apart)
    with pytest.raises(VtError, match="not contiguous"):
        Image.yv12(y, good, u)               # V first: U would have to follow it


# ---- packing host planes -------------------------------------------------------------------------------------------------------
def test_i420_buffer_and_separate_planes_pack_the_same_bytes():
    from vittracker_amd.native import Image, ImageTable, pack_image_offsets
    rs = np.random.RandomState(5)
    H, W = 6, 10
    y, u, v = oy.random_planes(rs, "i420", H, W)
    buf = np.concatenate([y.ravel(), u.ravel(), v.ravel()]).reshape(3 * H // 2, W)
    arenas = []
    for im in (Image.i420(y, u, v), Image.i420_buffer(buf)):
        offs, end = pack_image_offsets([im], start=48)
        (po,), rows = offs, im.plane_rows()
        assert len(po) == 2 and rows == [(H, W), (H, W // 2)]                    # one plane-1 offset for both chroma planes
        arena = np.zeros(end, np.uint8)
        for a, o, (n, rb) in zip(im.host_planes(), po, rows):
            arena[o:o + n * rb].reshape(n, rb)[...] = np.asarray(a).reshape(n, rb)
        d = im.descriptor([0x100000 + o for o in po], [rb for _, rb in rows])
        ImageTable.check(d[6], d[0], d[1], d[4], d[5], d[2], d[3], 0, nbytes0=end - po[0], nbytes1=end - po[1])
        arenas.append(arena)
        # the second chroma plane lies pitch1 * H/2 bytes after the first
        assert np.array_equal(arena[po[1] + (W // 2) * (H // 2):po[1] + (W // 2) * H].reshape(H // 2, W // 2), v)
    assert np.array_equal(arenas[0], arenas[1])


def test_p010_and_packed_layouts_pack_their_row_bytes():
    from vittracker_amd.native import Image, pack_image_offsets
    rs = np.random.RandomState(6)
    y, c = oy.random_planes(rs, "p010", 4, 6)
    ims = [Image.p010(y, c), Image.yuyv(oy.random_planes(rs, "yuyv", 3, 4)[0]), Image.gray(oy.random_planes(rs, "gray", 3, 5)[0])]
    offs, end = pack_image_offsets(ims, start=0)
    assert [im.plane_rows() for im in ims] == [[(4, 12), (2, 12)], [(3, 8)], [(3, 5)]]
    assert [len(o) for o in offs] == [2, 1, 1] and end == offs[2][0] + 15
    hp = ims[0].host_planes()
    assert hp[0].reshape(4, 12)[1, 3] == y[1, 1] >> 8 and hp[1].reshape(2, 12)[1, 5] == c[1, 1, 0] >> 8      # little-endian: high byte second
