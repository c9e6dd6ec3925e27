"""CPU: the wide layouts of vt_image -- YV16 / YV24, NV16 / NV24, P210 / P410 and the planar layouts in LSB-aligned 16-bit words (I010
... I416, GRAY10 / GRAY12 / GRAY16): the header's defines against the native constants, format_word round trips, ImageTable.check's
accept / reject matrix (colour bits, parity, doubled row bytes, the even-address rule of the 10- and 12-bit words, extents), the 8-bit
sample rule of the oracle against the I420 / I422 / I444 oracles, and the Image constructors with the arena's packing."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
import pixel_oracle_planar as opl
import pixel_oracle_wide as ow
import pixel_oracle_yuv as oy

P0, P1 = 0x10000, 0x20000
H, W = 34, 36


# ---- header, constants, format word ------------------------------------------------------------------------------------------------
def test_header_defines_equal_the_native_constants():
    from vittracker_amd import native
    src = open(os.path.join(REPO, "include", "vittrack.h")).read()
    defs = dict((k, int(v, 0)) for k, v in re.findall(r"#define VT_PIX_(\w+) (0x[0-9a-fA-F]+|\d+)\b", src))
    want = {"YV16": 21, "YV24": 22, "NV16": 23, "NV24": 24, "P210": 25, "P410": 26, "I010": 32, "I012": 33, "I016": 34, "I210": 36,
            "I212": 37, "I216": 38, "I410": 40, "I412": 41, "I416": 42, "GRAY10": 44, "GRAY12": 45, "GRAY16": 46}
    for name, code in want.items():
        assert defs[name] == code == getattr(native, "PIX_" + name) == ow.LAYOUT_CODE[name.lower()], name
        assert native.PIX_LAYOUT_NAMES[code] == name.lower() and native.pix_name(code) == name
    for si, s in enumerate(ow.SUBS):
        for di, d in enumerate(ow.DEPTHS):
            assert native.pix_wide(s, d) == 32 | si << 2 | di
    for never in ow.UNASSIGNED:
        assert never not in native.PIX_LAYOUT_NAMES and never not in defs.values()
    assert native.IMAGE_DTYPE.itemsize == 48
    # the "Not supported" line: what is left
    tail = src[src.index("Not supported:"):]
    tail = tail[:tail.index("pitch0 / pitch1")]
    assert "chroma interpolation" in tail and "BT.2020" in tail and "big-endian" in tail
    assert not any(w in tail for w in ("YV16", "NV16", "NV24", "16-bit planar"))


def test_format_word_round_trips():
    from vittracker_amd import native
    for lay, m, r in ow.COMBOS:
        word = native.pix_format(ow.LAYOUT_CODE[lay], m, r)
        assert word == ow.format_word(lay, m, r) < 1 << 16
        assert native.pix_fields(word) == (ow.LAYOUT_CODE[lay], ("bt601", "bt709").index(m), ("limited", "full").index(r), 0)
        assert native.pix_name(word) == lay.upper()


# ---- ImageTable.check --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(34, 36), (33, 35), (2, 2), (1, 1)])
def test_check_accepts_every_legal_combination(hw):
    from vittracker_amd.native import ImageTable
    for lay, m, r in ow.COMBOS:
        h, w = ow.fit_size(lay, *hw)
        if h < 1 or w < 1:
            continue
        word = ow.format_word(lay, m, r)
        r0, r1 = ow.row_bytes(lay, w)
        assert ImageTable.check(word, P0, P1, h, w) == (r0, r1)
        assert ImageTable.check(word, P0, P1, h, w, r0 + 6, r1 + 4 if r1 else 0) == (r0 + 6, r1 + 4 if r1 else 0)
        if lay in ow.WIDE_LSB:      # 16-bit words: even addresses
            assert ImageTable.check(word, P0 + 2, P1 + 6, h, w) == (r0, r1)
        else:                       # bytes and high bytes: any address, any pitch
            assert ImageTable.check(word, P0 + 1, P1 + 3, h, w, r0 + 5, r1 + 3 if r1 else 0) == (r0 + 5, r1 + 3 if r1 else 0)


def test_check_rejects_each_new_poison_case_with_a_message():
    from vittracker_amd.native import ImageTable, VtError
    ok = ImageTable.check
    for never in ow.UNASSIGNED:
        with pytest.raises(VtError, match="unknown pixel format"):
            ok(never, P0, P1, H, W)
    for lay in ow.WIDE_LAYOUTS:
        word = ow.format_word(lay)
        r0, r1 = ow.row_bytes(lay, W)
        ok(word, P0, P1, H, W)
        with pytest.raises(VtError, match="null"):
            ok(word, 0, P1, H, W)
        with pytest.raises(VtError, match="shorter than a row"):
            ok(word, P0, P1, H, W, r0 - 2, 0)
        with pytest.raises(VtError, match="reserved"):
            ok(word, P0, P1, H, W, reserved=1)
        with pytest.raises(VtError, match="unknown pixel format"):
            ok(word | 1 << 16, P0, P1, H, W)
        for bits in (2 << 8, 2 << 12):
            with pytest.raises(VtError, match="unknown pixel format"):
                ok(word | bits, P0, P1, H, W)
        if r1:
            with pytest.raises(VtError, match="null"):
                ok(word, P0, 0, H, W)
            with pytest.raises(VtError, match="shorter than a row"):
                ok(word, P0, P1, H, W, 0, r1 - 2)
        else:
            ok(word, P0, 0, H, W)               # a grey image has no plane 1
            for m, r in oy.COLOURS[1:]:
                with pytest.raises(VtError, match="no matrix or range"):
                    ok(ow.LAYOUT_CODE[lay] | oy.format_word("rgb", m, r), P0, 0, H, W)
        # parity of the subsampling
        s = ow.sub_of(lay)
        if s == "420":
            for hw in ((H - 1, W), (H, W - 1)):
                with pytest.raises(VtError, match="even H and W"):
                    ok(word, P0, P1, *hw)
        elif s == "422":
            ok(word, P0, P1, H - 1, W)
            with pytest.raises(VtError, match="even W"):
                ok(word, P0, P1, H, W - 1)
        else:
            ok(word, P0, P1, H - 1, W - 1)
        # a row pitch of the 8-bit layout's bytes is half a row of 16-bit samples
        if ow.depth_of(lay) > 8:
            with pytest.raises(VtError, match="shorter than a row"):
                ok(word, P0, P1, H, W, W, 0)
        # 10- and 12-bit words: aligned 16-bit loads
        if lay in ow.WIDE_LSB:
            with pytest.raises(VtError, match="odd"):
                ok(word, P0 + 1, P1, H, W)
            with pytest.raises(VtError, match="odd"):
                ok(word, P0, P1, H, W, r0 + 1, 0)
            if r1:
                with pytest.raises(VtError, match="odd"):
                    ok(word, P0, P1 + 1, H, W)
                with pytest.raises(VtError, match="odd"):
                    ok(word, P0, P1, H, W, 0, r1 + 1)


def test_extents_are_pitch_times_rows_minus_one_plus_row_bytes():
    from vittracker_amd.native import ImageTable, VtError
    for lay in ow.WIDE_LAYOUTS:
        word = ow.format_word(lay)
        r0, r1 = ow.row_bytes(lay, W)
        for extra in (0, 6):
            q0, q1 = r0 + extra, (r1 + extra if r1 else 0)
            e0, e1 = ow.extents(lay, H, W, q0, q1)
            assert e0 == q0 * (H - 1) + r0 and (e1 == q1 * (ow.plane1_rows(lay, H) - 1) + r1 if r1 else e1 == 0)
            assert ImageTable.check(word, P0, P1, H, W, q0, q1, nbytes0=e0, nbytes1=e1 or None) == (q0, q1)
            with pytest.raises(VtError, match=f"plane 0: needs {e0} bytes"):
                ImageTable.check(word, P0, P1, H, W, q0, q1, nbytes0=e0 - 1, nbytes1=e1 or None)
            if r1:
                with pytest.raises(VtError, match=f"plane 1: needs {e1} bytes"):
                    ImageTable.check(word, P0, P1, H, W, q0, q1, nbytes0=e0, nbytes1=e1 - 1)
    # rows of plane 1: both chroma planes of the three-plane layouts, H rows of pairs
    assert [ow.plane1_rows(lay, H) for lay in ("yv16", "yv24", "nv16", "nv24", "p210", "p410", "i010", "i210", "i410")] == \
        [2 * H, 2 * H, H, H, H, H, H, 2 * H, 2 * H]
    assert [ow.row_bytes(lay, W) for lay in ("yv16", "yv24", "nv16", "nv24", "p210", "p410", "i010", "i210", "i410", "gray12")] == \
        [(W, W // 2), (W, W), (W, W), (W, 2 * W), (2 * W, 2 * W), (2 * W, 4 * W), (2 * W, W), (2 * W, W), (2 * W, 2 * W), (2 * W, 0)]
    # ... inside a 32-bit offset: 2 H - 1 rows of I410's plane 1 count, not H - 1
    q = 1 << 26
    assert q * (H - 1) + 2 * W <= 0xfffffff0 < q * (2 * H - 1) + 2 * W
    ImageTable.check(ow.format_word("nv24"), P0, P1, H, W, 0, q)
    with pytest.raises(VtError, match="beyond the 32-bit offsets"):
        ImageTable.check(ow.format_word("i410"), P0, P1, H, W, 0, q)


# ---- the 8-bit sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", ow.DEPTHS)
def test_words_of_any_low_bits_denote_the_image_of_their_top_eight_bits(depth):
    """An I0xx / I2xx / I4xx image whose words are s8 << (depth - 8) | r has, for any r, the rgb(d) of the I420 / I422 / I444 image of
    s8; 16 bits: through the high byte."""
    rs = np.random.RandomState(depth)
    for sub, stem in (("420", "i0"), ("422", "i2"), ("444", "i4")):
        lay = stem + str(depth)
        ch, cw = ow.chroma_shape(lay, H, W)
        Y, U, V = (rs.randint(0, 256, s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        for m, r in oy.COLOURS:
            want = oy.rgb_of("i420", [Y, U, V], m, r) if sub == "420" else opl.rgb_of("i" + sub, [Y, U, V], m, r)
            for junk in (None, rs, rs):
                pl = ow.planes_of_yuv(lay, Y, U, V, junk)
                assert all(p.dtype == np.uint16 and int(p.max()) < 1 << depth for p in pl)
                assert np.array_equal(ow.rgb_of(lay, pl, m, r), want), (lay, m, r)
            if depth == 16:
                hi = [p.view(np.uint8)[..., 1::2] for p in ow.planes_of_yuv(lay, Y, U, V, rs)]
                assert all(np.array_equal(a, b) for a, b in zip(hi, (Y, U, V)))
    g = rs.randint(0, 256, (H, W)).astype(np.uint8)
    assert np.array_equal(ow.rgb_of("gray%d" % depth, ow.planes_of_yuv("gray%d" % depth, g, None, None, rs)), oy.rgb_of("gray", [g]))


def test_the_byte_and_high_byte_layouts_denote_their_planar_twins():
    rs = np.random.RandomState(5)
    for lay, twin in (("yv16", "i422"), ("yv24", "i444"), ("nv16", "i422"), ("nv24", "i444"), ("p210", "i422"), ("p410", "i444")):
        ch, cw = ow.chroma_shape(lay, H, W)
        Y, U, V = (rs.randint(0, 256, s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        pl = ow.planes_of_yuv(lay, Y, U, V, rs)
        for m, r in oy.COLOURS:
            assert np.array_equal(ow.rgb_of(lay, pl, m, r), opl.rgb_of(twin, [Y, U, V], m, r)), (lay, m, r)
    # V first; pairs are (U, V)
    Y, U, V = np.full((2, 2), 81, np.uint8), np.full((2, 1), 90, np.uint8), np.full((2, 1), 240, np.uint8)      # red, BT.601 limited
    for lay in ("yv16", "nv16", "p210", "i210", "i212", "i216"):
        assert ow.rgb_of(lay, ow.planes_of_yuv(lay, Y, U, V))[0, 0].tolist() == oy.yuv_to_rgb(81, 90, 240)[()].tolist() == [254, 0, 0]
    assert ow.planes_of_yuv("yv16", Y, U, V)[1][0, 0] == 240 and ow.planes_of_yuv("nv16", Y, U, V)[1][0, 0].tolist() == [90, 240]
    assert ow.planes_of_yuv("p210", Y, U, V)[1][0, 0].tolist() == [90 << 8, 240 << 8]


def test_a_word_above_the_range_saturates():
    for depth in (10, 12):
        top = 255 << (depth - 8) | ((1 << (depth - 8)) - 1)
        words = np.array([0, 1 << (depth - 8), top, top + 1, 1 << depth, 0x7fff, 0x8000, 0xffff], np.uint16)
        assert ow.s8(words, depth).tolist() == [0, 1, 255, 255, 255, 255, 255, 255]
        assert ow.rgb_of("gray%d" % depth, [words.reshape(2, 4)]).reshape(-1, 3)[:, 0].tolist() == [0, 1, 255, 255, 255, 255, 255, 255]
    assert ow.s8(np.array([0x00ff, 0x0100, 0xff00, 0xffff], np.uint16), 16).tolist() == [0, 1, 255, 255]
    # int16 storage is the same bits
    assert ow.s8(np.array([-1, -32768], np.int16), 10).tolist() == [255, 255]


def test_planes_of_rgb_come_back_close_on_444():
    rs = np.random.RandomState(9)
    rgb = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    for lay in ("i410", "yv24", "p410"):
        back = ow.rgb_of(lay, ow.planes_of_rgb(lay, rgb, "bt709", "full", rs), "bt709", "full")
        assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 2      # two roundings to 8 bits


# ---- constructors ------------------------------------------------------------------------------------------------------------------
def _stacked(a, b, extra=0):
    """Two equal-shaped planes back to back in one array at a row pitch `extra` samples wider than the row."""
    n = a.shape[0]
    buf = np.zeros((2 * n, a.shape[1] + extra), a.dtype)
    buf[:n, :a.shape[1]], buf[n:, :a.shape[1]] = a, b
    return buf[:n, :a.shape[1]], buf[n:, :a.shape[1]]


def test_constructors_give_the_words_pitches_and_rows():
    from vittracker_amd import native
    from vittracker_amd.native import Image, ImageTable
    rs = np.random.RandomState(13)
    for lay, m, r in ow.COMBOS[::3] + [c for c in ow.COMBOS if c[0] in ow.WIDE_GRAY]:
        h, w = ow.fit_size(lay, 33, 35)
        pl = ow.random_planes(rs, lay, h, w)
        kind, d = ow.LAYOUTS[lay][2], ow.depth_of(lay)
        if kind in ("v3", "p3"):
            pl[1], pl[2] = _stacked(pl[1], pl[2], 3)
        if kind == "g":
            im = Image.gray16(pl[0], depth=d)
        elif kind == "p3":
            im = Image.yuv16(*pl, depth=d, sub=ow.sub_of(lay), matrix=m, range=r)
        else:
            im = getattr(Image, lay)(*pl, matrix=m, range=r)
        r0, r1 = ow.row_bytes(lay, w)
        b = 2 if d > 8 else 1
        assert (im.format, im.H, im.W) == (ow.format_word(lay, m, r), h, w)
        assert im.pitches == ((r0,) if kind == "g" else (r0, r1 + 3 * b if kind in ("v3", "p3") else r1))
        assert im.plane_rows() == [(h, r0)] + ([(ow.plane1_rows(lay, h), r1)] if r1 else [])
        hp = im.host_planes()
        assert len(hp) == (2 if r1 else 1) and all(a.dtype == np.uint8 for a in hp)
        # what the arena packs is what the oracle reads
        flat = [np.ascontiguousarray(np.asarray(a).reshape(n, -1)[:, :rb]) for a, (n, rb) in zip(hp, im.plane_rows())]
        back = [f.view(np.uint16) if d > 8 else f for f in flat]
        ch, cw = ow.chroma_shape(lay, h, w) if r1 else (0, 0)
        if kind in ("v3", "p3"):
            back = [back[0], back[1][:ch], back[1][ch:]]
        elif kind == "sp":
            back = [back[0], back[1].reshape(ch, cw, 2)]
        assert np.array_equal(ow.rgb_of(lay, back, m, r), ow.rgb_of(lay, pl, m, r))
        offs, end = native.pack_image_offsets([im], start=48)
        d_ = im.descriptor([0x100000 + o for o in offs[0]], [rb for _, rb in im.plane_rows()])
        ImageTable.check(d_[6], d_[0], d_[1], d_[4], d_[5], d_[2], d_[3], 0, nbytes0=end, nbytes1=end if r1 else None)


def test_i010_shorthand_and_input_types():
    import torch
    from vittracker_amd.native import Image, VtError
    rs = np.random.RandomState(17)
    y, u, v = ow.random_planes(rs, "i010", 4, 6)
    u, v = _stacked(u, v)
    a = Image.i010(y, u, v, matrix="bt709")
    assert (a.format, a.H, a.W, a.pitches, a.plane_rows()) == (32 | 1 << 8, 4, 6, (12, 6), [(4, 12), (4, 6)])
    b = Image.yuv16(y.view(np.int16), u.view(np.int16), v.view(np.int16), depth=10, sub="420", matrix="bt709")
    c = Image.yuv16(y.view(np.uint8), u.view(np.uint8), v.view(np.uint8), depth=10, sub="420", matrix="bt709")
    for o in (b, c):
        assert (o.format, o.H, o.W, o.pitches) == (a.format, 4, 6, (12, 6))
    ty = torch.from_numpy(y.view(np.int16).copy())
    tc = torch.from_numpy(np.concatenate([u, v]).view(np.int16).copy())
    t = Image.i010(ty, tc[:2], tc[2:])
    assert (t.format, t.H, t.W, t.pitches) == (32, 4, 6, (12, 6))
    g = Image.gray16(torch.from_numpy(y.view(np.int16).copy()), depth=12)
    assert (g.format, g.H, g.W, g.pitches, g.plane_rows()) == (45, 4, 6, (12,), [(4, 12)])
    with pytest.raises(VtError, match="not back to back"):
        Image.i010(y, u.copy(), np.zeros((4, 3), np.uint16)[2:])      # two allocations: V is not pitch1 * H/2 behind U
    with pytest.raises(VtError, match="depth"):
        Image.yuv16(y, u, v, depth=14)
    with pytest.raises(VtError, match="sub"):
        Image.yuv16(y, u, v, sub="gray")
    with pytest.raises(VtError, match="W even"):
        Image.nv16(np.zeros((4, 5), np.uint8), np.zeros((4, 2, 2), np.uint8))
    with pytest.raises(VtError, match="chroma plane must be"):
        Image.p410(np.zeros((4, 5), np.uint16), np.zeros((4, 4, 2), np.uint16))
    n24 = Image.nv24(np.zeros((3, 5), np.uint8), np.zeros((3, 5, 2), np.uint8))
    assert (n24.format, n24.pitches, n24.plane_rows()) == (24, (5, 10), [(3, 5), (3, 10)])
    p4 = Image.p410(np.zeros((3, 5), np.uint16), np.zeros((3, 5, 2), np.uint16), range="full")
    assert (p4.format, p4.pitches, p4.plane_rows()) == (26 | 1 << 12, (10, 20), [(3, 10), (3, 20)])
