"""CPU: the planar layouts of vt_image (RGBP / BGRP, I444, I422) -- the header's defines against the native constants and the ctypes
struct, ImageTable.check's accept / reject matrix (colour bits, pitches, the no-alignment rule, the pitch1 (2 H - 1) + row extent), the
Image constructors (strides taken from views, CHW tensors, permuted HWC views, planes that are not back to back) and the numpy oracle
against the I420 oracle and against plain transposition."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
import pixel_oracle_planar as op
import pixel_oracle_yuv as oy

P0, P1 = 0x10000, 0x20000
SIZES = [(97, 131), (64, 48), (33, 35)]


def _even(W):
    return W - W % 2


# ---- header, constants, struct -------------------------------------------------------------------------------------------------
def test_header_defines_native_constants_and_struct_agree():
    from vittracker_amd import native
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    defs = dict((k, int(v, 0)) for k, v in re.findall(r"#define VT_PIX_(\w+) (0x[0-9a-fA-F]+|\d+)\b", src))
    assert {k: defs[k] for k in ("RGBP", "BGRP", "I444", "I422")} == {
        "RGBP": native.PIX_RGBP, "BGRP": native.PIX_BGRP, "I444": native.PIX_I444, "I422": native.PIX_I422} == {
        "RGBP": 16, "BGRP": 17, "I444": 18, "I422": 19}
    assert "#define VT_PIX_LAYOUT(format) ((format) & 0xff)" in src
    names = native.PIX_LAYOUT_NAMES
    assert (names[16], names[17], names[18], names[19]) == ("rgbp", "bgrp", "i444", "i422")
    for never in (6, 7, 14, 15):
        assert never not in names and never not in defs.values()
    assert native.PIX_NAMES[:6] == ("rgb", "bgr", "rgba", "bgra", "nv12", "nv21")
    for lay, code in op.LAYOUT_CODE.items():
        for mi, m in enumerate(("bt601", "bt709")):
            for ri, r in enumerate(("limited", "full")):
                assert native.pix_format(code, m, r) == op.format_word(lay, m, r) == code | (mi << 8) | (ri << 12)
    # the struct did not change: two plane pointers, two pitches, four int32, 48 bytes in this order
    body = re.search(r"typedef struct vt_image \{(.*?)\} vt_image;", src, re.S).group(1)
    ct = {"const uint8_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const uint8_t\*|int64_t|int32_t)\s+(.*)", decl)
        fields += [(n.strip().lstrip("*"), ct[m.group(1)]) for n in m.group(2).split(",")]
    S = type("S", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(S) == 48 == native.IMAGE_DTYPE.itemsize
    assert [f[0] for f in fields] == list(native.IMAGE_DTYPE.names) == ["plane0", "plane1", "pitch0", "pitch1", "H", "W", "format", "reserved"]
    assert "4:4:4 layouts" not in src and all(w in src for w in ("YV16", "NV16", "16-bit planar"))


# ---- ImageTable.check ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SIZES)
def test_check_accepts_every_legal_word(hw):
    from vittracker_amd.native import ImageTable
    H, W0 = hw
    for lay, m, r in op.COMBOS:
        W = _even(W0) if lay == "i422" else W0
        cw = op.chroma_width(lay, W)
        word = op.format_word(lay, m, r)
        assert ImageTable.check(word, P0, P1, H, W) == (W, cw)                                   # pitch 0 = the row's bytes
        assert ImageTable.check(word, P0, P1, H, W, W + 5, cw + 3) == (W + 5, cw + 3)            # padded, odd pitches
        for a0, a1 in ((1, 0), (0, 1), (3, 2), (0, H * W)):                                      # no alignment rule, plane1 of odd CHW
            assert ImageTable.check(word, P0 + a0, P1 + a1, H, W) == (W, cw)
        # the buffers' sizes: plane1 covers both trailing planes
        need1 = (cw + 3) * (2 * H - 1) + cw
        assert ImageTable.check(word, P0, P1, H, W, W, cw + 3, nbytes0=W * H, nbytes1=need1) == (W, cw + 3)


def test_check_rejects_each_poison_case():
    from vittracker_amd.native import ImageTable, VtError
    H, W = 33, 36
    ok = lambda *a, **k: ImageTable.check(*a, **k)      # noqa: E731
    for lay in op.PLANAR_LAYOUTS:
        word = op.format_word(lay)
        cw = op.chroma_width(lay, W)
        ok(word, P0, P1, H, W)
        with pytest.raises(VtError, match="null"):
            ok(word, 0, P1, H, W)
        with pytest.raises(VtError, match="null"):
            ok(word, P0, 0, H, W)
        with pytest.raises(VtError, match="shorter than a row"):
            ok(word, P0, P1, H, W, W - 1, 0)
        with pytest.raises(VtError, match="shorter than a row"):
            ok(word, P0, P1, H, W, 0, cw - 1)
        with pytest.raises(VtError, match="reserved"):
            ok(word, P0, P1, H, W, reserved=1)
        with pytest.raises(VtError):
            ok(word | (1 << 16), P0, P1, H, W)
        with pytest.raises(VtError):
            ok(word | (2 << 8), P0, P1, H, W)
        with pytest.raises(VtError):
            ok(word, P0, P1, 0, W)
    for lay in ("rgbp", "bgrp"):                        # colour bits belong to the YUV layouts
        for m, r in oy.COLOURS[1:]:
            with pytest.raises(VtError, match="no matrix or range"):
                ok(op.LAYOUT_CODE[lay] | oy.format_word("rgb", m, r), P0, P1, H, W)
    with pytest.raises(VtError, match="even W"):
        ok(op.format_word("i422"), P0, P1, H, W - 1)
    for lay in ("rgbp", "bgrp", "i444"):                # odd W and H are fine on the three others, odd H on I422
        ok(op.format_word(lay), P0, P1, H, W - 1)
    ok(op.format_word("i422"), P0, P1, H, W)
    for never in (14, 15, 20):
        with pytest.raises(VtError, match="unknown pixel format"):
            ok(never, P0, P1, H, W)


def test_extent_of_plane1_is_pitch1_times_2h_minus_1_plus_row():
    from vittracker_amd.native import ImageTable, VtError
    H, W = 33, 36
    for lay in op.PLANAR_LAYOUTS:
        word, cw = op.format_word(lay), op.chroma_width(lay, W)
        for pitch1 in (cw, cw + 7):
            need = pitch1 * (2 * H - 1) + cw
            ok = ImageTable.check(word, P0, P1, H, W, 0, pitch1, nbytes0=W * H, nbytes1=need)
            assert ok == (W, pitch1)
            with pytest.raises(VtError, match=f"plane 1: needs {need} bytes"):
                ImageTable.check(word, P0, P1, H, W, 0, pitch1, nbytes0=W * H, nbytes1=need - 1)
        with pytest.raises(VtError, match="plane 0: needs"):
            ImageTable.check(word, P0, P1, H, W, nbytes0=W * H - 1, nbytes1=1 << 20)
    # ... and it must fit the kernels' 32-bit offsets: 2 H rows count, not H
    Hb, Wb = 40000, 30000
    ImageTable.check(op.format_word("i444"), P0, P1, Hb, Wb)                       # 2.4e9 bytes: fits
    with pytest.raises(VtError, match="plane 1: .* beyond the 32-bit offsets"):
        ImageTable.check(op.format_word("i444"), P0, P1, 80000, Wb)                # plane 0 fits (2.4e9), both trailing planes do not
    ImageTable.check(op.format_word("i422"), P0, P1, 80000, Wb)                    # half-width chroma: fits again


# ---- constructors --------------------------------------------------------------------------------------------------------------
def _addr(a):
    return a.__array_interface__["data"][0]


@pytest.mark.parametrize("hw", SIZES)
def test_chw_takes_pointers_and_strides_from_the_view(hw):
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import Image
    H, W = hw
    rs = np.random.RandomState(H)
    a = rs.randint(0, 256, (3, H, W)).astype(np.uint8)
    for order, code in (("rgb", native.PIX_RGBP), ("bgr", native.PIX_BGRP)):
        im = Image.chw(a, order)
        assert (im.format, im.H, im.W, im.pitches) == (code, H, W, (W, W)) and im.shape == (H, W, 3)
        assert [_addr(p) for p in im.planes] == [_addr(a) + k * H * W for k in range(3)]
        d = im.descriptor([_addr(p) for p in im.planes], im.pitches)
        assert d == (_addr(a), _addr(a) + H * W, W, W, H, W, code, 0)
        native.ImageTable.check(d[6], d[0], d[1], d[4], d[5], d[2], d[3])          # plane1 at an odd address for 33 x 35
    # a CPU tensor, and rows padded to a pitch with the planes pitch * H apart
    t = torch.from_numpy(a)
    assert Image.chw(t).pitches == (W, W) and Image.chw(t).planes[1].data_ptr() == t.data_ptr() + H * W
    wide = rs.randint(0, 256, (3, H, W + 9)).astype(np.uint8)
    im = Image.chw(wide[:, :, :W])
    assert im.pitches == (W + 9, W + 9) and _addr(im.planes[2]) - _addr(im.planes[1]) == (W + 9) * H
    assert np.array_equal(np.stack(im.host_planes()[1].reshape(2, H, W)), wide[1:, :, :W])
    assert im.plane_rows() == [(H, W), (2 * H, W)]
    # a window of fewer rows: the planes are no longer pitch * H apart, which one pitch and one pointer cannot say
    with pytest.raises(native.VtError, match="back to back"):
        Image.chw(wide[:, 1:, :W])
    with pytest.raises(native.VtError, match="dense"):
        Image.chw(wide[:, :, ::2])
    with pytest.raises(native.VtError, match=r"\(3, H, W\)"):
        Image.chw(a.transpose(1, 2, 0))
    with pytest.raises(native.VtError, match="order"):
        Image.chw(a, "gbr")
    with pytest.raises(native.VtError, match="uint8"):
        Image.chw(a.astype(np.float32))


def test_chw_of_a_permuted_hwc_view_is_the_packed_frame():
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import Image
    rs = np.random.RandomState(2)
    hwc = rs.randint(0, 256, (33, 35, 3)).astype(np.uint8)
    for view in (hwc.transpose(2, 0, 1), torch.from_numpy(hwc).permute(2, 0, 1)):
        im = Image.chw(view)
        assert (im.format, im.H, im.W, im.pitches, len(im.planes)) == (native.PIX_RGB, 33, 35, (105,), 1)
        assert Image._address(im.planes[0]) == _addr(hwc)
        assert Image.chw(view, "bgr").format == native.PIX_BGR


def test_three_plane_constructors_want_back_to_back_planes():
    from vittracker_amd import native
    from vittracker_amd.native import Image, VtError
    rs = np.random.RandomState(3)
    H, W = 33, 36
    buf = rs.randint(0, 256, (3, H, W + 4)).astype(np.uint8)
    r, g, b = (buf[k, :, :W] for k in range(3))
    for mk, code in ((Image.rgb_planar, native.PIX_RGBP), (Image.bgr_planar, native.PIX_BGRP), (Image.i444, native.PIX_I444)):
        im = mk(r, g, b)
        assert (im.format, im.H, im.W, im.pitches) == (code, H, W, (W + 4, W + 4))
    # plane 0 has a pointer and a pitch of its own: it may lie anywhere
    r2 = np.ascontiguousarray(r)
    assert Image.rgb_planar(r2, g, b).pitches == (W, W + 4)
    assert Image.i444(r2, g, b, matrix="bt709", range="full").format == native.PIX_I444 | 0x1100
    # the trailing planes may not: separate allocations, swapped order, two pitches
    with pytest.raises(VtError, match="back to back"):
        Image.rgb_planar(r, np.ascontiguousarray(g), np.ascontiguousarray(b))
    with pytest.raises(VtError, match="back to back"):
        Image.rgb_planar(r, b, g)
    with pytest.raises(VtError, match="one row pitch"):
        Image.rgb_planar(r, g, np.ascontiguousarray(b))
    with pytest.raises(VtError, match="must be"):
        Image.rgb_planar(r, g, b[:, :-1])
    # I422: chroma planes of W / 2 columns, W even
    c = rs.randint(0, 256, (2, H, W // 2 + 3)).astype(np.uint8)
    im = Image.i422(r2, c[0, :, :W // 2], c[1, :, :W // 2], matrix="bt709")
    assert (im.format, im.pitches, im.plane_rows()) == (native.PIX_I422 | 0x100, (W, W // 2 + 3), [(H, W), (2 * H, W // 2)])
    with pytest.raises(VtError, match="W even"):
        Image.i422(r2[:, :-1], c[0, :, :W // 2], c[1, :, :W // 2])
    with pytest.raises(VtError, match="must be"):
        Image.i422(r2, g, b)


def test_images_from_chw_shares_memory():
    import torch
    from vittracker_amd import native
    rs = np.random.RandomState(4)
    B, H, W = 3, 33, 35
    batch = rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    for src in (batch, torch.from_numpy(batch)):
        ims = native.images_from_chw(src)
        assert len(ims) == B and all(im.format == native.PIX_RGBP and im.shape == (H, W, 3) for im in ims)
        for k, im in enumerate(ims):
            assert [native.Image._address(p) for p in im.planes] == [_addr(batch) + (3 * k + c) * H * W for c in range(3)]
    ims = native.images_from_chw(batch, order="bgr")
    batch[1, 2, 5, 7] ^= 0xff                                # no copy: the Image sees the write
    assert int(ims[1].planes[2][5, 7]) == int(batch[1, 2, 5, 7]) and ims[1].format == native.PIX_BGRP
    with pytest.raises(native.VtError, match=r"\(B, 3, H, W\)"):
        native.images_from_chw(batch.transpose(0, 2, 3, 1))


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 48), (34, 36)])
def test_oracle_against_the_i420_oracle_and_transposition(hw):
    H, W = hw
    rs = np.random.RandomState(H + W)
    y, u, v = oy.random_planes(rs, "i420", H, W)
    for m, r in oy.COLOURS:
        want = oy.rgb_of("i420", [y, u, v], m, r)
        up = lambda a, fy, fx: np.repeat(np.repeat(a, fy, axis=0), fx, axis=1)      # noqa: E731
        assert np.array_equal(op.rgb_of("i444", [y, up(u, 2, 2), up(v, 2, 2)], m, r), want)
        assert np.array_equal(op.rgb_of("i422", [y, up(u, 2, 1), up(v, 2, 1)], m, r), want)
    frame = rs.randint(0, 256, (H + 1, W + 1, 3)).astype(np.uint8)                   # odd sizes
    chw = np.ascontiguousarray(frame.transpose(2, 0, 1))
    assert np.array_equal(op.rgb_of("rgbp", list(chw)), frame)
    assert np.array_equal(op.rgb_of("bgrp", list(chw[::-1])), frame)
    # arbitrary pitches and offsets: plane1 at an odd offset, the third plane pitch1 * H behind it
    Hh, Ww = H + 1, W + 1
    p0, p1 = Ww + 3, Ww + 6
    b0 = rs.randint(0, 256, 5 + p0 * Hh).astype(np.uint8)
    b1 = rs.randint(0, 256, 7 + p1 * 2 * Hh).astype(np.uint8)
    got = op.rgb_of_buffers("rgbp", b0, p0, b1, p1, Hh, Ww, off0=5, off1=7)
    assert got[4, 9].tolist() == [b0[5 + 4 * p0 + 9], b1[7 + 4 * p1 + 9], b1[7 + (Hh + 4) * p1 + 9]]
    got = op.rgb_of_buffers("i422", b0, p0, b1, p1, Hh, W, "bt709", "full", off0=5, off1=7)
    assert got[4, 9].tolist() == oy.yuv_to_rgb(b0[5 + 4 * p0 + 9], b1[7 + 4 * p1 + 4], b1[7 + (Hh + 4) * p1 + 4], "bt709", "full").tolist()
