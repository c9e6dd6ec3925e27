"""GPU: the layouts and colour rows added to vt_image -- I420 / YV12, YUYV / UYVY, P010, GRAY8, and BT.709 / full range for every YUV
layout, NV12 / NV21 included -- each held bit for bit to what the *_frames entry points compute on a tight RGB frame holding rgb(d),
the numpy oracle's conversion (tests/pixel_oracle_yuv.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import pixel_oracle
import pixel_oracle_yuv as oy
from test_gpu_frame_formats import MEAN, STD, _dev_plane, _model, _params

pytestmark = pytest.mark.gpu

# both dimensions even; narrow planes (guarded windows), a plane of one chroma row, one frame larger than the crops
SIZES = [(2, 2), (6, 4), (34, 2), (10, 12), (36, 54), (200, 302), (64, 64), (128, 128)]
PITCH = [0, 3, 0, 8, 0, 5, 0, 0]       # extra bytes per row of every plane (odd: rows at unaligned offsets)
NBOX = 6
NEW_YUV = ("i420", "yv12", "yuyv", "uyvy", "p010")
COMBOS = [(lay, m, r) for lay in NEW_YUV for (m, r) in oy.COLOURS] + \
         [(lay, m, r) for lay in ("nv12", "nv21") for (m, r) in oy.COLOURS[1:]] + [("gray", "bt601", "limited")]
OLD = pixel_oracle.FORMATS


def _box(kind, H, W):
    """Boxes hanging over each of the four edges, one whose crop covers the whole frame (its valid range ends at the last row and
    column: P010's guarded windows, I420's last chroma row) and one too small (poisoned in both routes)."""
    if kind == 0:
        return [-0.3 * W, 0.2 * H, 0.6 * W, 0.5 * H]          # left
    if kind == 1:
        return [0.2 * W, -0.3 * H, 0.5 * W, 0.6 * H]          # top
    if kind == 2:
        return [0.7 * W, 0.3 * H, 0.6 * W, 0.5 * H]           # right
    if kind == 3:
        return [0.3 * W, 0.7 * H, 0.5 * W, 0.6 * H]           # bottom
    if kind == 4:
        return [0.0, 0.0, float(W), float(H)]                 # all of it, and over every edge at factor 2
    return [0.5 * W, 0.5 * H, 0.0, 0.0]                       # too small


def _image(layout, planes, extra, matrix="bt601", rng="limited"):
    """A device Image of host planes, every plane in an allocation that ends at its last byte, rows `extra` bytes apart beyond the row."""
    from vittracker_amd.native import Image
    if layout in OLD and layout not in ("nv12", "nv21"):
        return getattr(Image, layout)(_dev_plane(planes[0], extra)[0])
    if layout == "gray":
        return Image.gray(_dev_plane(planes[0], extra)[0])
    kw = dict(matrix=matrix, range=rng)
    if layout in ("yuyv", "uyvy"):
        return getattr(Image, layout)(_dev_plane(planes[0], extra)[0], **kw)
    if layout == "p010":      # the uint8 views of the 16-bit planes
        return Image.p010(_dev_plane(planes[0].view(np.uint8), extra)[0], _dev_plane(planes[1].view(np.uint8), extra)[0], **kw)
    if layout in ("i420", "yv12"):      # the two chroma planes back to back at one pitch, in one allocation
        H2 = planes[1].shape[0]
        c = _dev_plane(np.concatenate([planes[1], planes[2]], axis=0), extra)[0]
        return getattr(Image, layout)(_dev_plane(planes[0], extra)[0], c[:H2], c[H2:], **kw)
    return getattr(Image, layout)(*[_dev_plane(a, extra)[0] for a in planes], **kw)


def _rgb(layout, planes, matrix, rng):
    return pixel_oracle.rgb_of(layout, planes) if layout in OLD and (matrix, rng) == oy.COLOURS[0] else oy.rgb_of(layout, planes, matrix, rng)


_PLANES = {}


def _planes(layout, k):
    """Host planes of `layout` at SIZES[k]: made once, shared by every test and colour row."""
    if (layout, k) not in _PLANES:
        rs = np.random.RandomState(1000 + 16 * sorted(oy.LAYOUT_CODE).index(layout) + k)
        H, W = SIZES[k]
        _PLANES[(layout, k)] = pixel_oracle.random_planes(rs, layout, H, W) if layout in OLD else oy.random_planes(rs, layout, H, W)
    return _PLANES[(layout, k)]


def _same(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _check_crops(combos, crop_sizes):
    """Every combo at every size, under NBOX boxes each: crop_u8_images / crop_images == crop_u8_frames / crop_frames on rgb(d), resize
    factors included (NaN where the box is too small)."""
    import torch
    from vittracker_amd.native import FrameTable, ImageTable
    ims, frames, boxes, what = [], [], [], []
    for (lay, m, r) in combos:
        for k, (H, W) in enumerate(SIZES):
            pl = _planes(lay, k)
            im, fr = _image(lay, pl, PITCH[k], m, r), torch.from_numpy(_rgb(lay, pl, m, r)).cuda()
            for kind in range(NBOX):
                ims.append(im), frames.append(fr), boxes.append(_box(kind, H, W)), what.append((lay, m, r, H, W, kind))
    B = len(ims)
    mdl = _model(128, B)
    itab, ftab = ImageTable.of(ims), FrameTable.of(frames)
    st = torch.tensor(boxes, dtype=torch.float64).cuda()
    for T in crop_sizes:
        p8, r8 = mdl.crop_u8_images(itab, st, 2.0, T)
        q8, s8 = mdl.crop_u8_frames(ftab, st, 2.0, T)
        pf, rf = mdl.crop_images(itab, st, 2.0, T, MEAN, STD)
        qf, sf = mdl.crop_frames(ftab, st, 2.0, T, MEAN, STD)
        assert _same(r8, s8) and _same(rf, sf), T
        small = torch.isnan(s8).cpu().numpy()
        assert small.sum() == B // NBOX and bool(torch.isnan(qf[torch.isnan(sf)]).all())
        bad8 = (p8 != q8).flatten(1).any(1).cpu().numpy()
        badf = (pf.view(torch.int32) != qf.view(torch.int32)).flatten(1).any(1).cpu().numpy()
        assert not bad8.any() and not badf.any(), (T, [what[i] for i in np.nonzero(bad8 | badf)[0][:8]])


@pytest.mark.parametrize("combo", COMBOS, ids=["-".join(c) for c in COMBOS])
def test_every_combination_crops_like_its_rgb_frame(combo):
    """T = 64 (a band size; at this batch the generic kernel) and T = 37 (odd: scalar stores), both outputs."""
    _check_crops([combo], (64, 37))


@pytest.mark.parametrize("env", [{"VT_CROP_BAND": "-4"}, {"VT_CROP_BAND": "-2"}])
def test_band_forms_crop_like_the_rgb_frames(env):
    """crop_band_image_kernel with 4 and 2 items per thread, forced in a child (a process reads the switches once): every combination,
    T = 64 and 128."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_frame_formats_yuv as T
T._check_crops(T.COMBOS, (64, 128))
print("FORM-OK")
""" % (REPO, os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FORM-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_a_table_mixing_old_and_new_layouts_crops_each_frame_alone():
    """B = 24: the six old layouts and every new one, colour tags varied; T = 64 runs the generic kernel, T = 256 the band kernel.
    Each sequence equals that sequence cropped alone (B = 1: the generic kernel)."""
    import torch
    from vittracker_amd.native import ImageTable
    mix = [(f, "bt601", "limited") for f in OLD] + [COMBOS[(7 * i) % len(COMBOS)] for i in range(17)] + [("gray", "bt601", "limited")]
    assert len(mix) == 24 and {c[0] for c in mix} >= set(OLD) | set(NEW_YUV) | {"gray"} and len({c[1:] for c in mix}) == 4
    ims, boxes = [], []
    for i, (lay, m, r) in enumerate(mix):
        k = 3 + i % 5
        ims.append(_image(lay, _planes(lay, k), PITCH[k], m, r))
        boxes.append(_box(i % 5, *SIZES[k]))
    B = len(ims)
    mdl, one = _model(128, B), _model(128, 1)
    st = torch.tensor(boxes, dtype=torch.float64).cuda()
    itab = ImageTable.of(ims)
    for T in (64, 256):
        p8, r8 = mdl.crop_u8_images(itab, st, 2.0, T)
        pf, rf = mdl.crop_images(itab, st, 2.0, T, MEAN, STD)
        for b in range(B):
            t1 = ImageTable.of([ims[b]])
            a8, ar = one.crop_u8_images(t1, st[b:b + 1], 2.0, T)
            af, _ = one.crop_images(t1, st[b:b + 1], 2.0, T, MEAN, STD)
            assert torch.equal(p8[b], a8[0]) and float(r8[b]) == float(ar[0]) == float(rf[b]), (T, b, mix[b])
            assert torch.equal(pf[b].view(torch.int32), af[0].view(torch.int32)), (T, b, mix[b])


def test_unusable_descriptors_poison_their_own_sequence_only():
    """One unusable descriptor per rule of the header; every other sequence stays bit-identical (T = 64 / 37: generic, 256: band)."""
    import torch
    from vittracker_amd.native import ImageTable
    H, W = 40, 52
    rs = np.random.RandomState(3)
    lays = ["i420", "rgb", "gray", "yuyv", "p010", "yv12", "uyvy", "nv12"] * 3
    ims = [_image(f, (pixel_oracle if f in OLD else oy).random_planes(rs, f, H, W), 0) for f in lays]
    B = len(ims)
    mdl = _model(128, B)
    boxes = torch.tensor([[5.0, 6.0, 20.0, 15.0]] * B, dtype=torch.float64).cuda()
    good = ImageTable.of(ims)
    bad = ImageTable(B, "cuda")
    for i, im in enumerate(ims):
        bad.set_image(i, im)
    poison = {}

    def spoil(i, **kw):
        d = dict(zip(bad.DTYPE.names, bad.host[i].tolist()))
        d.update(kw)
        bad.set(i, tuple(d[n] for n in bad.DTYPE.names), check=False)
        poison[i] = kw

    spoil(0, format=7)                                          # never assigned
    spoil(1, format=0 | 1 << 8)                                 # a matrix on RGB
    spoil(2, format=13 | 1 << 12)                               # a range on GRAY8
    spoil(3, W=W - 1)                                           # YUYV odd W
    spoil(4, pitch1=2 * W - 2)                                  # P010: a chroma row is 2 W bytes
    spoil(5, H=H - 1)                                           # YV12 odd H
    spoil(6, format=14)                                         # beyond the last layout
    spoil(7, format=4 | 1 << 16)                                # a bit in 16-31
    spoil(8, pitch1=W // 2 - 1)                                 # I420 short chroma pitch
    spoil(9, format=6)
    spoil(10, format=13 | 1 << 8)                               # a matrix on GRAY8
    spoil(12, W=W - 1)                                          # P010 odd W
    spoil(13, plane1=0)                                         # YV12 without chroma
    spoil(14, format=11 | 2 << 8)                               # matrix 2
    spoil(15, format=4 | 2 << 12)                               # range 2
    spoil(16, plane1=int(bad.host[16]["plane1"]) + 2)           # I420 chroma misaligned
    spoil(20, pitch0=2 * W - 1)                                 # P010: a luma row is 2 W bytes
    bad.upload()
    for T in (64, 37, 256):
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
                assert not np.isnan(float(r8[b]))


STEP_FORMS = [("p010", "bt709", "limited"), ("i420", "bt601", "full")]


@pytest.mark.parametrize("geom,B", [(128, 1), (128, 7), (128, 256), (256, 7)])
def test_image_step_equals_the_frame_step(geom, B):
    """vt_track_step_images on P010 / 709-limited and I420 / 601-full == vt_track_step_frames on the oracle's RGB: records and states,
    closed loop over 3 steps."""
    import torch
    from vittracker_amd.native import FrameTable, ImageTable, Outputs
    n = 3
    rs = np.random.RandomState(80 + B)
    sizes = [(96, 128), (150, 212), (72, 100), (60, 40)]
    pool = []          # a few distinct frames per form, cycled over steps and sequences
    for j in range(8):
        lay, m, r = STEP_FORMS[j % 2]
        H, W = sizes[(j // 2) % 4]
        pl = oy.random_planes(rs, lay, H, W)
        pool.append((_image(lay, pl, 4 * (j % 2), m, r), torch.from_numpy(oy.rgb_of(lay, pl, m, r)).cuda()))
    mdl = _model(geom, B)
    mdl.set_template(torch.from_numpy(rs.standard_normal((B, 3, geom // 2, geom // 2)).astype(np.float32)).cuda())
    box0 = torch.tensor([[rs.uniform(0, 30), rs.uniform(0, 20), rs.uniform(10, 30), rs.uniform(10, 25)] for _ in range(B)],
                        dtype=torch.float64).cuda()
    box0[0] = torch.tensor([30.0, 50.0, 30.0, 20.0], dtype=torch.float64)       # reaches the last rows of the 60 x 40 frame
    x = torch.empty(B, 3, geom, geom, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, geom // 16, "cuda")
    ftab, itab = FrameTable(B, "cuda"), ImageTable(B, "cuda")

    def run(images):
        st = box0.clone()
        recs, states = [], []
        for t in range(n):
            rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
            for b in range(B):
                im, fr = pool[(3 * t + b + (6 if b == 0 else 0)) % 8]
                itab.set_image(b, im) if images else ftab.set_tensor(b, fr)
            if images:
                itab.upload()
                mdl.track_step_images(itab, st, 4.0, MEAN, STD, x, rf, out, record=rec)
            else:
                ftab.upload()
                mdl.track_step_frames(ftab, st, 4.0, MEAN, STD, x, rf, out, record=rec)
            recs.append(rec)
            states.append(st.clone())
        return torch.stack(recs), torch.stack(states)

    want = run(False)
    got = run(True)
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_batched_tracker_on_host_i420_and_device_p010_equals_it_on_the_rgb_frames():
    """Three frames: host I420 (three planes, and the one-buffer form) through the pinned arena and device P010 give the records of the
    converted RGB frames."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    p = _params("vit_48_h32_g128")
    B, n = 4, 3
    rs = np.random.RandomState(90)
    sizes = [(240, 320), (120, 160), (72, 100), (130, 96)]
    seq = []
    for t in range(n + 1):
        row = []
        for b in range(B):
            H, W = sizes[b]
            i4, p10 = oy.random_planes(rs, "i420", H, W), oy.random_planes(rs, "p010", H, W)
            row.append({"i420": i4, "p010": p10, "rgb_i420": oy.rgb_of("i420", i4, "bt709", "limited"), "rgb_p010": oy.rgb_of("p010", p10, "bt709", "full")})
        seq.append(row)
    boxes = [[W * 0.3, H * 0.3, max(2.0, W * 0.2), max(2.0, H * 0.2)] for H, W in sizes]
    boxes[1] = [150.0, 110.0, 14.0, 9.0]             # clipped at its frame's edge

    def run(kind):
        def frame(t, b):
            s = seq[t][b]
            if kind.startswith("rgb"):
                return s[kind]
            if kind == "i420":
                y, u, v = s["i420"]
                if b % 2:
                    return Image.i420_buffer(np.concatenate([y.ravel(), u.ravel(), v.ravel()]).reshape(-1, y.shape[1]), matrix="bt709")
                return Image.i420(y, u, v, matrix="bt709")
            y, c = s["p010"]
            return Image.p010(torch.from_numpy(y.view(np.int16)).cuda(), torch.from_numpy(c.view(np.int16)).cuda(), matrix="bt709", range="full")
        bt = BatchedVitTracker(p, B)
        bt.initialize([frame(0, b) for b in range(B)], boxes)
        return np.stack([bt.track_record([frame(t, b) for b in range(B)]) for t in range(1, n + 1)])

    assert np.array_equal(run("i420"), run("rgb_i420"))
    assert np.array_equal(run("p010"), run("rgb_p010"))


def test_plugin_on_gray_and_yuyv_images_equals_it_on_the_rgb_frames():
    from vittracker_amd.native import Image
    from vittracker_amd.tracker.vit_dist import get_tracker_class
    p = _params("vit_48_h32_noKD")
    rs = np.random.RandomState(95)
    H, W = 150, 206
    box = {"init_bbox": [60.0, 40.0, 30.0, 24.0]}
    for lay, mk in (("gray", lambda a: Image.gray(a)), ("yuyv", lambda a: Image.yuyv(a, matrix="bt709", range="full"))):
        raw = [oy.random_planes(rs, lay, H, W)[0] for _ in range(4)]
        rgb = [oy.rgb_of(lay, [a], "bt709", "full") for a in raw]
        a, b = get_tracker_class()(p, "synthetic"), get_tracker_class()(p, "synthetic")
        a.initialize(rgb[0], box)
        b.initialize(mk(raw[0]), box)
        for f, g in zip(rgb[1:], raw[1:]):
            assert a.track(f) == b.track(mk(g)), lay


def test_ostrack_step_on_nv12_bt709_equals_it_on_the_rgb_frames():
    """One ViT-Base step at B = 2 through BatchedVitTracker with the ostrack parameters: NV12 tagged BT.709 against its RGB frames."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitb_256")
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    rs = np.random.RandomState(97)
    H, W = 180, 240
    pl = [[pixel_oracle.random_planes(rs, "nv12", H, W) for _ in range(2)] for _ in range(2)]
    rgb = [[oy.rgb_of("nv12", q, "bt709", "limited") for q in row] for row in pl]
    boxes = [[80.0, 60.0, 40.0, 30.0], [200.0, 150.0, 30.0, 24.0]]
    recs = []
    for images in (False, True):
        bt = BatchedVitTracker(p, 2)
        bt.initialize([rgb[0][b] for b in range(2)], boxes)
        fr = [Image.nv12(torch.from_numpy(pl[1][b][0]).cuda(), torch.from_numpy(pl[1][b][1]).cuda(), matrix="bt709") if images else rgb[1][b]
              for b in range(2)]
        recs.append(bt.track_record(fr))
    assert np.isfinite(recs[0]).all() and np.array_equal(recs[0], recs[1])
