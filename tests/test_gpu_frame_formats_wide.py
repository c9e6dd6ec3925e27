"""GPU: the wide layouts of vt_image -- YV16 / YV24, NV16 / NV24, P210 / P410 and the planar 16-bit layouts (I010 ... I416, GRAY10 /
GRAY12 / GRAY16) -- each, under all four colour rows where it is a YUV layout, held bit for bit to what the *_frames entry points compute
on a tight RGB frame holding rgb(d), the numpy oracle's image (tests/pixel_oracle_wide.py): crops on both routes, B = 1, the tracker
step, a mixed table, unusable descriptors, a captured step replayed over I010 <-> I420 descriptors, BatchedVitTracker.  Frames of
34 x 36 and (where odd sizes are legal) 33 x 35 at padded pitches; the padding is 0xFF and the bits below every sample are random, so
wrong addressing or a missing shift shows as wrong values.  No tolerance anywhere: every comparison is of bits."""
import numpy as np
import pytest

import pixel_oracle_wide as ow
import pixel_oracle_yuv as oy
from test_gpu_frame_formats import MEAN, STD, _model, _params
from test_gpu_frame_formats_planar import _box, _run_steps, _same, NBOX

pytestmark = pytest.mark.gpu

SIZES = [(34, 36), (33, 35)]
CROPS = (64, 37, 256)      # band size / odd (general kernel, scalar stores) / band size
B = len(ow.COMBOS)         # 15 YUV layouts x 4 colour rows + 3 grey layouts = 63


def _extra(layout, k):
    """Padding bytes a row: even for the 10- / 12-bit words (aligned 16-bit loads), odd for the layouts read as single bytes."""
    return 6 if layout in ow.WIDE_LSB else (5, 3)[k]


def _dev(a, extra):
    """A device copy of host plane `a` (viewed as bytes) in an allocation of its own that ENDS at the plane's last byte, rows `extra`
    bytes apart beyond the row's bytes, the padding 0xFF."""
    import torch
    a8 = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    rows, rb = a8.shape
    pitch = rb + extra
    flat = torch.full((pitch * (rows - 1) + rb,), 0xff, dtype=torch.uint8, device="cuda")
    v = torch.as_strided(flat, (rows, rb), (pitch, 1))
    v.copy_(torch.from_numpy(a8))
    return v


def _image(layout, planes, extra, matrix="bt601", rng="limited", as16=False):
    """A device Image of host planes as pixel_oracle_wide lays them out: plane 0 in an allocation of its own, the two trailing planes of
    a three-plane layout back to back at one pitch in another.  as16: 16-bit planes go in as int16 tensors, else as their byte views."""
    import torch
    from vittracker_amd.native import Image
    _, sub, kind, d = ow.LAYOUTS[layout]
    w = (lambda t: t.view(torch.int16)) if (as16 and d > 8 and extra % 2 == 0) else (lambda t: t)
    kw = dict(matrix=matrix, range=rng)
    y = _dev(planes[0], extra)
    if kind == "g":
        return Image.gray16(w(y), depth=d)
    if kind == "sp":
        ch, cw = planes[1].shape[:2]
        c = _dev(planes[1], extra)
        e = c.shape[1] // cw                 # bytes a pair
        return getattr(Image, layout)(w(y), w(torch.as_strided(c, (ch, cw, e), (c.stride(0), e, 1))), **kw)
    ch = planes[1].shape[0]
    c = _dev(np.concatenate([planes[1], planes[2]], axis=0), extra)
    if kind == "v3":
        return getattr(Image, layout)(y, c[:ch], c[ch:], **kw)
    return Image.yuv16(w(y), w(c[:ch]), w(c[ch:]), depth=d, sub=sub, **kw)


_CASES = {}


def _case(combo, k):
    """(device Image, the oracle's RGB frame on the device) of a combination at SIZES[k] (made legal for its subsampling): made once,
    shared by every test."""
    import torch
    if (combo, k) not in _CASES:
        lay, m, r = combo
        H, W = ow.fit_size(lay, *SIZES[k])
        rs = np.random.RandomState(3000 + 4 * ow.COMBOS.index(combo) + k)
        pl = ow.random_planes(rs, lay, H, W)
        _CASES[(combo, k)] = (_image(lay, pl, _extra(lay, k), m, r, as16=k == 0), torch.from_numpy(ow.rgb_of(lay, pl, m, r)).cuda())
    return _CASES[(combo, k)]


def _compare(mdl, ims, frames, boxes, crop_sizes, what):
    """crop_u8_images / crop_images == crop_u8_frames / crop_frames on the RGB frames, patches and resize factors."""
    import torch
    from vittracker_amd.native import FrameTable, ImageTable
    itab, ftab = ImageTable.of(ims), FrameTable.of(frames)
    st = torch.tensor(boxes, dtype=torch.float64).cuda()
    for T in crop_sizes:
        p8, r8 = mdl.crop_u8_images(itab, st, 2.0, T)
        q8, s8 = mdl.crop_u8_frames(ftab, st, 2.0, T)
        pf, rf = mdl.crop_images(itab, st, 2.0, T, MEAN, STD)
        qf, sf = mdl.crop_frames(ftab, st, 2.0, T, MEAN, STD)
        assert _same(r8, s8) and _same(rf, sf) and bool(torch.isfinite(s8).all()), T
        bad8 = (p8 != q8).flatten(1).any(1).cpu().numpy()
        badf = (pf.view(torch.int32) != qf.view(torch.int32)).flatten(1).any(1).cpu().numpy()
        assert not bad8.any() and not badf.any(), (T, [what[i] for i in np.nonzero(bad8 | badf)[0][:8]])
        assert int(q8.to(torch.int64).sum()) > 0


def _table(k, shift):
    ims, frames, boxes, what = [], [], [], []
    for i, combo in enumerate(ow.COMBOS):
        im, fr = _case(combo, k)
        kind = (i + shift) % NBOX
        ims.append(im), frames.append(fr), boxes.append(_box(kind, im.H, im.W)), what.append(combo + (im.H, im.W, kind))
    return ims, frames, boxes, what


@pytest.mark.parametrize("k", range(len(SIZES)), ids=["34x36", "33x35"])
def test_every_combination_crops_like_its_rgb_frame(k):
    """One table of all 63 layout x colour combinations; boxes hang over every edge and corner, shifted so that each layout meets
    several.  B = 63: T = 64 and 37 take the general kernel, T = 256 the band kernel (4 items a thread for the uint8 patch, 2 for the
    fp32 crop).  The table three times over, B = 189, is enough items for the band kernel at T = 64 (2 items) and T = 128 (4 / 2)."""
    mdl = _model(128, B)
    for shift in (0, 3, 7):
        ims, frames, boxes, what = _table(k, shift)
        _compare(mdl, ims, frames, boxes, CROPS, what)
    ims, frames, boxes, what = (sum((_table(k, s)[j] for s in (1, 4, 8)), []) for j in range(4))
    _compare(_model(128, 3 * B), ims, frames, boxes, (64, 128), what)


def test_b_equals_1_takes_the_single_item_route():
    m1 = _model(128, 1)
    for k in range(len(SIZES)):
        ims, frames, boxes, what = _table(k, 1)
        for i in range(k, B, 4):      # every layout at least once, colour rows alternating
            _compare(m1, ims[i:i + 1], frames[i:i + 1], boxes[i:i + 1], (128, 37), what[i:i + 1])


def test_samples_are_the_top_eight_bits_whatever_lies_below():
    """I010 / I212 / I416 / P210 / GRAY12 frames of the same samples with zero, all-ones and random low bits crop alike."""
    import torch
    from vittracker_amd.native import ImageTable
    rs = np.random.RandomState(41)
    H, W = 34, 36
    lays = ("i010", "i212", "i416", "p210", "gray12")
    ims = []
    for lay in lays:
        ch, cw = ow.chroma_shape(lay, H, W)
        Y, U, V = (rs.randint(0, 256, s).astype(np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        for junk in ("zero", "ones", "random"):
            pl = ow.planes_of_yuv(lay, Y, U, V, rs if junk == "random" else None)
            if junk == "ones":
                d = ow.depth_of(lay)
                pl = [(p | ((1 << (d - 8)) - 1)).astype(p.dtype) for p in pl]
            ims.append(_image(lay, pl, 6, "bt709", "limited") if lay != "gray12" else _image(lay, pl, 6))
    mdl = _model(128, len(ims))
    st = torch.tensor([_box(i % NBOX, H, W) for i in range(len(lays)) for _ in range(3)], dtype=torch.float64).cuda()
    for T in CROPS:
        p8, _ = mdl.crop_u8_images(ImageTable.of(ims), st, 2.0, T)
        for i in range(len(lays)):
            assert torch.equal(p8[3 * i], p8[3 * i + 1]) and torch.equal(p8[3 * i], p8[3 * i + 2]), (T, lays[i])
            assert int(p8[3 * i].to(torch.int64).sum()) > 0


def test_step_on_every_combination_equals_the_frame_step():
    """vt_track_step_images on the table of 63 == vt_track_step_frames on the RGB frames: G128, two steps on two tables."""
    import torch
    from vittracker_amd.native import FrameTable, ImageTable
    geom, n = 128, 2
    rs = np.random.RandomState(43)
    mdl = _model(geom, B)
    mdl.set_template(torch.from_numpy(rs.standard_normal((B, 3, geom // 2, geom // 2)).astype(np.float32)).cuda())
    tabs = [_table(k, 2) for k in range(n)]
    box0 = torch.tensor([_box((i + 2) % NBOX, 33, 34) for i in range(B)], dtype=torch.float64).cuda()
    want = _run_steps(mdl, geom, B, box0, n, [FrameTable.of(t[1]) for t in tabs], False)
    got = _run_steps(mdl, geom, B, box0, n, [ImageTable.of(t[0]) for t in tabs], True)
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_mixed_table_of_old_and_new_layouts():
    """RGB, I010 / 709, NV12, P210 / full, I420, GRAY16, I444, NV24, YV16 / 709 full, P010, I412: the general kernel at T = 37, the band
    kernel at T = 256 (the eleven rows six times over)."""
    import torch
    import pixel_oracle
    import pixel_oracle_planar as opl
    from test_gpu_frame_formats_planar import _image as planar_image
    from test_gpu_frame_formats_yuv import _image as yuv_image
    rs = np.random.RandomState(45)
    H, W = 34, 36
    rows = []
    for lay, m, r in (("rgb", None, None), ("i010", "bt709", "limited"), ("nv12", "bt601", "limited"), ("p210", "bt601", "full"),
                      ("i420", "bt709", "full"), ("gray16", "bt601", "limited"), ("i444", "bt601", "limited"), ("nv24", "bt601", "limited"),
                      ("yv16", "bt709", "full"), ("p010", "bt709", "limited"), ("i412", "bt601", "full")):
        if lay in ow.LAYOUTS:
            rows.append(_case((lay, m, r), 0))
        elif lay in opl.LAYOUT_CODE:
            pl = opl.random_planes(rs, lay, H, W)
            rows.append((planar_image(lay, pl, 3, m, r), torch.from_numpy(opl.rgb_of(lay, pl, m, r)).cuda()))
        elif lay == "rgb":
            pl = pixel_oracle.random_planes(rs, lay, H, W)
            rows.append((yuv_image(lay, pl, 4), torch.from_numpy(pixel_oracle.rgb_of(lay, pl)).cuda()))
        else:
            pl = oy.random_planes(rs, lay, H, W)
            rows.append((yuv_image(lay, pl, 4, m, r), torch.from_numpy(oy.rgb_of(lay, pl, m, r)).cuda()))
    for sel, crops in ((list(range(11)), (37, 80)), (list(range(11)) * 6, (128, 256))):
        ims, frames = [rows[i][0] for i in sel], [rows[i][1] for i in sel]
        boxes = [_box((2 * i + 1) % NBOX, im.H, im.W) for i, im in enumerate(ims)]
        _compare(_model(128, len(sel)), ims, frames, boxes, crops, sel)


def test_unusable_descriptors_poison_their_own_sequence_only():
    """One unusable descriptor per new rule of the header in the table of 63 good ones; each bad descriptor's planes point one past the
    end of a small allocation with extents that would be legal, so a kernel that read through it would read outside it."""
    import torch
    from vittracker_amd.native import ImageTable
    ims, _, _, _ = _table(0, 0)
    H, W = 34, 36
    mdl = _model(128, B)
    boxes = torch.tensor([_box(8, H, W)] * B, dtype=torch.float64).cuda()
    good = ImageTable.of(ims)
    bad = ImageTable(B, "cuda")
    for i, im in enumerate(ims):
        bad.set_image(i, im)
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    end = small.data_ptr() + small.numel()
    assert end % 2 == 0
    poison = {}

    def at(lay, n=0):
        return [i for i, c in enumerate(ow.COMBOS) if c[0] == lay][n]

    def spoil(i, **kw):
        assert i not in poison
        d = dict(zip(bad.DTYPE.names, bad.host[i].tolist()))
        d.update(plane0=end, plane1=end, pitch0=0, pitch1=0)
        d.update(kw)
        bad.set(i, tuple(d[n] for n in bad.DTYPE.names), check=False)
        poison[i] = kw

    for n, code in enumerate((35, 39, 43, 47)):                  # dep = 3
        spoil(at("i016", n), format=code)
    for n, code in enumerate((27, 28, 29, 30)):                  # never assigned
        spoil(at("i216", n), format=code)
    spoil(at("i416", 0), format=31)
    spoil(at("i416", 1), format=48)                              # beyond the last layout
    spoil(at("i416", 2), format=20)
    spoil(at("i416", 3), format=127)
    spoil(at("i010", 0), plane0=end + 1)                         # 10-bit words at an odd address ...
    spoil(at("i010", 1), plane1=end + 1)
    spoil(at("i012", 0), pitch0=2 * W + 1)                       # ... or at an odd pitch
    spoil(at("i412", 0), pitch1=2 * W + 1)
    spoil(at("gray10"), plane0=end + 1)
    spoil(at("gray12"), pitch0=2 * W + 3)
    spoil(at("i010", 2), H=H - 1)                                # parity of 4:2:0 ...
    spoil(at("i010", 3), W=W - 1)
    spoil(at("i012", 1), W=W - 1)
    spoil(at("i210", 0), W=W - 1)                                # ... and of 4:2:2
    spoil(at("i212", 0), W=W - 1)
    spoil(at("nv16", 0), W=W - 1)
    spoil(at("p210", 0), W=W - 1)
    spoil(at("yv16", 0), W=W - 1)
    spoil(at("i012", 2), pitch0=W)                               # a pitch of the 8-bit row: half a row of words
    spoil(at("i210", 1), pitch1=W - 2)
    spoil(at("p210", 1), pitch0=2 * W - 1)
    spoil(at("p410", 0), pitch1=4 * W - 1)
    spoil(at("nv24", 0), pitch1=2 * W - 1)
    spoil(at("nv16", 1), pitch1=W - 1)
    spoil(at("yv24", 0), pitch1=W - 1)
    spoil(at("gray16"), pitch0=2 * W - 1)
    spoil(at("i410", 0), pitch1=1 << 26)                         # 2 H - 1 = 67 rows of 2^26 bytes do not fit 32 bits (33 would)
    spoil(at("p410", 1), pitch0=1 << 32)
    spoil(at("i410", 1), plane1=0)
    spoil(at("nv24", 1), plane1=0)
    spoil(at("yv24", 1), plane0=0)
    spoil(at("i410", 2), format=40 | 2 << 8)                     # matrix 2
    spoil(at("i410", 3), format=40 | 2 << 12)                    # range 2
    spoil(at("nv16", 2), format=23 | 1 << 16)                    # a bit in 16-31
    spoil(at("p210", 2), reserved=1)
    assert int(bad.host[at("i410", 0)]["pitch1"]) * (H - 1) + 2 * W <= 0xfffffff0 < int(bad.host[at("i410", 0)]["pitch1"]) * (2 * H - 1) + 2 * W
    # colour bits on a grey layout: GRAY16's row is taken, so GRAY10's word goes onto another good row
    spoil(at("yv16", 1), format=44 | 1 << 8)
    spoil(at("yv16", 2), format=46 | 1 << 12)
    bad.upload()
    for T in CROPS:
        ref8, rr8 = mdl.crop_u8_images(good, boxes, 2.0, T)
        reff, rrf = mdl.crop_images(good, boxes, 2.0, T, MEAN, STD)
        p8, r8 = mdl.crop_u8_images(bad, boxes, 2.0, T)
        pf, rf = mdl.crop_images(bad, boxes, 2.0, T, MEAN, STD)
        for b in range(B):
            if b in poison:
                assert np.isnan(float(r8[b])) and np.isnan(float(rf[b])), (T, b, poison[b])
                assert int(p8[b].abs().sum()) == 0 and bool(torch.isnan(pf[b]).all()), (T, b, poison[b])
            else:
                assert torch.equal(p8[b], ref8[b]) and float(r8[b]) == float(rr8[b]) and torch.equal(pf[b], reff[b]), (T, b)
                assert not np.isnan(float(r8[b])) and int(p8[b].to(torch.int64).sum()) > 0


def test_captured_step_replays_over_a_table_rewritten_from_i010_to_i420_and_back():
    import torch
    from test_gpu_frame_formats_yuv import _image as yuv_image
    from vittracker_amd.native import FrameTable, ImageTable, Outputs
    geom, Bc = 128, 4
    rs = np.random.RandomState(47)
    H, W = 34, 36
    rows = []
    for t in range(3):      # I010 (random junk below the samples), the I420 frames of other samples, I010 again
        ims, frames = [], []
        for b in range(Bc):
            Y, U, V = (rs.randint(0, 256, s).astype(np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
            m, r = oy.COLOURS[(t + b) % 4]
            if t == 1:
                ims.append(yuv_image("i420", [Y, U, V], 4, m, r))
                frames.append(torch.from_numpy(oy.rgb_of("i420", [Y, U, V], m, r)).cuda())
            else:
                pl = ow.planes_of_yuv("i010", Y, U, V, rs)
                ims.append(_image("i010", pl, 6, m, r))
                frames.append(torch.from_numpy(ow.rgb_of("i010", pl, m, r)).cuda())
                assert np.array_equal(ow.rgb_of("i010", pl, m, r), oy.rgb_of("i420", [Y, U, V], m, r))
        rows.append((ims, frames))
    mdl = _model(geom, Bc)
    mdl.set_template(torch.from_numpy(rs.standard_normal((Bc, 3, geom // 2, geom // 2)).astype(np.float32)).cuda())
    box0 = torch.tensor([[10.0, 8.0, 14.0, 12.0], [20.0, 15.0, 12.0, 10.0], [2.0, 3.0, 18.0, 14.0], [12.0, 9.0, 10.0, 16.0]],
                        dtype=torch.float64).cuda()
    want = _run_steps(mdl, geom, Bc, box0, 3, [FrameTable.of(r[1]) for r in rows], False)
    x, rf, out = torch.empty(Bc, 3, geom, geom, device="cuda"), torch.empty(Bc, dtype=torch.float64, device="cuda"), Outputs(Bc, geom // 16, "cuda")
    st, rec = box0.clone(), torch.empty(Bc, 5, dtype=torch.float64, device="cuda")
    itab = ImageTable(Bc, "cuda")
    for b in range(Bc):
        itab.set_image(b, rows[0][0][b])
    itab.upload()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        mdl.track_step_images(itab, st, 4.0, MEAN, STD, x, rf, out, record=rec, stream=torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(side)
    st.copy_(box0)
    got = []
    for ims, _ in rows:
        for b in range(Bc):
            itab.set_image(b, ims[b])        # the same table address, other formats, pointers and pitches
        itab.upload()
        g.replay()
        got.append(rec.clone())
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(torch.stack(got), want[0]) and torch.equal(st, want[1][-1])


def test_batched_tracker_on_i010_frames_equals_it_on_the_rgb_frames():
    """Host uint16 planes (packed into the pinned arena at doubled row bytes) and device int16 tensors give the records of the converted
    RGB frames."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    p = _params("vit_48_h32_g128")
    Bt, n = 4, 3
    rs = np.random.RandomState(49)
    sizes = [(34, 36), (72, 100), (120, 160), (40, 6)]
    seq = []
    for t in range(n + 1):
        row = []
        for H, W in sizes:
            y, u, v = ow.random_planes(rs, "i010", H, W)
            c = np.concatenate([u, v], axis=0)      # back to back
            row.append((y, c[:H // 2], c[H // 2:], ow.rgb_of("i010", [y, u, v], "bt709", "limited")))
        seq.append(row)
    boxes = [[W * 0.3, H * 0.3, max(2.0, W * 0.2), max(2.0, H * 0.2)] for H, W in sizes]

    def run(kind):
        def frame(t, b):
            y, u, v, rgb = seq[t][b]
            if kind == "rgb":
                return rgb
            if kind == "host":
                return Image.i010(y, u, v, matrix="bt709")
            c = torch.from_numpy(np.concatenate([u, v], axis=0).view(np.int16)).cuda()
            return Image.i010(torch.from_numpy(y.view(np.int16)).cuda(), c[:u.shape[0]], c[u.shape[0]:], matrix="bt709")
        bt = BatchedVitTracker(p, Bt)
        bt.initialize([frame(0, b) for b in range(Bt)], boxes)
        return np.stack([bt.track_record([frame(t, b) for b in range(Bt)]) for t in range(1, n + 1)])

    want = run("rgb")
    assert np.isfinite(want).all()
    assert np.array_equal(run("dev"), want)
    assert np.array_equal(run("host"), want)
