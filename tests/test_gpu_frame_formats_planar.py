"""GPU: the planar layouts of vt_image -- RGBP / BGRP (the CHW tensors of PyTorch dataloaders), I444 and I422 -- each held bit for bit to
what the *_frames entry points compute on a tight RGB frame holding rgb(d), the numpy oracle's image (tests/pixel_oracle_planar.py):
the crops on every route (general kernel, band kernel with 2 and 4 items a thread, B = 1), unusable descriptors, the tracker step of a
vit_dist and of a family="vit" model, a captured step replayed over rewritten tables, BatchedVitTracker and the plugin.  No tolerance
anywhere: every comparison is of bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import pixel_oracle
import pixel_oracle_planar as op
import pixel_oracle_yuv as oy
from test_gpu_frame_formats import MEAN, STD, _dev_plane, _model, _params

pytestmark = pytest.mark.gpu

SIZES = [(97, 131), (64, 48), (33, 35)]      # odd H and W (I422: W - 1), one frame smaller than the crops
PITCH = [0, 5, 3]                            # extra bytes per row of every plane (odd: rows and planes at unaligned offsets)
NBOX = 9


def _size(layout, k):
    H, W = SIZES[k]
    return H, (W - W % 2 if layout == "i422" else W)


def _box(kind, H, W):
    """Boxes hanging over each of the four borders and the four corners, and one wholly inside (factor 2: the crop is twice the box)."""
    w, h = 0.3 * W, 0.3 * H
    cx = {0: 0.0, 1: 0.5 * W, 2: W - 1.0}
    cy = {0: 0.0, 1: 0.5 * H, 2: H - 1.0}
    i, j = [(0, 1), (2, 1), (1, 0), (1, 2), (0, 0), (2, 0), (0, 2), (2, 2), (1, 1)][kind]
    if kind == 8:
        w, h = 0.2 * W, 0.2 * H
    return [cx[i] - 0.5 * w, cy[j] - 0.5 * h, w, h]


def _image(layout, planes, extra, matrix="bt601", rng="limited"):
    """A device Image of three host planes: plane 0 in an allocation of its own, the two trailing planes back to back at one pitch in
    another; both allocations END at their plane's last byte, rows `extra` bytes apart beyond the row."""
    from vittracker_amd.native import Image
    H = planes[0].shape[0]
    a = _dev_plane(planes[0], extra)[0]
    c = _dev_plane(np.concatenate([planes[1], planes[2]], axis=0), extra)[0]
    if layout == "rgbp":
        return Image.rgb_planar(a, c[:H], c[H:])
    if layout == "bgrp":
        return Image.bgr_planar(a, c[:H], c[H:])
    return getattr(Image, layout)(a, c[:H], c[H:], matrix=matrix, range=rng)


_CASES = {}


def _case(combo, k):
    """(device Image, the oracle's RGB frame on the device) of a combination at SIZES[k]: made once, shared by every test."""
    import torch
    if (combo, k) not in _CASES:
        lay, m, r = combo
        H, W = _size(lay, k)
        rs = np.random.RandomState(2000 + 16 * op.COMBOS.index(combo) + k)
        pl = op.random_planes(rs, lay, H, W)
        _CASES[(combo, k)] = (_image(lay, pl, PITCH[k], m, r), torch.from_numpy(op.rgb_of(lay, pl, m, r)).cuda())
    return _CASES[(combo, k)]


def _same(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


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


def _check_crops(combos, crop_sizes, one=False):
    ims, frames, boxes, what = [], [], [], []
    for combo in combos:
        for k in range(len(SIZES)):
            im, fr = _case(combo, k)
            for kind in range(NBOX):
                ims.append(im), frames.append(fr), boxes.append(_box(kind, im.H, im.W)), what.append(combo + (im.H, im.W, kind))
    mdl = _model(128, len(ims))
    _compare(mdl, ims, frames, boxes, crop_sizes, what)
    if one:      # B = 1: every descriptor alone
        m1 = _model(128, 1)
        for i in range(0, len(ims), 4):
            _compare(m1, ims[i:i + 1], frames[i:i + 1], boxes[i:i + 1], (128, 80), what[i:i + 1])


@pytest.mark.parametrize("combo", op.COMBOS, ids=["-".join(c) for c in op.COMBOS])
def test_every_combination_crops_like_its_rgb_frame(combo):
    """The general kernel: T = 80, T = 37 (odd: scalar stores) and, at this batch of 27, the band size T = 64; then B = 1 at T = 128, 80."""
    _check_crops([combo], (80, 37, 64), one=True)


def test_band_kernel_crops_like_the_rgb_frames():
    """All ten combinations in one table of 270: every band size takes the band kernel in the form the batch picks."""
    _check_crops(op.COMBOS, (64, 128, 256))


@pytest.mark.parametrize("env", [{"VT_CROP_BAND": "-4"}, {"VT_CROP_BAND": "-2"}])
def test_band_forms_crop_like_the_rgb_frames(env):
    """crop_band_image_kernel with 4 and 2 items per thread, forced in a child (a process reads the switches once)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_frame_formats_planar as T
T._check_crops(T.op.COMBOS, (64, 128, 256))
print("FORM-OK")
""" % (REPO, os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FORM-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_mixed_tables_crop_like_their_rgb_frames():
    """B = 5: RGBP, NV12, I444 / 709 full, RGB, I422 / 601 full, and a second order with I420 -- the general kernel at T = 80 and 256;
    B = 42, the six rows seven times over: the band kernel at T = 128 and 256."""
    import torch
    from test_gpu_frame_formats_yuv import _image as yuv_image
    rs = np.random.RandomState(7)
    rows = [(_case(("rgbp", "bt601", "limited"), 0)), None, _case(("i444", "bt709", "full"), 2), None, _case(("i422", "bt601", "full"), 0), None]
    for i, lay in ((1, "nv12"), (3, "rgb"), (5, "i420")):
        pl = (pixel_oracle if lay in pixel_oracle.FORMATS else oy).random_planes(rs, lay, 64, 48)
        rgb = pixel_oracle.rgb_of(lay, pl) if lay in pixel_oracle.FORMATS else oy.rgb_of(lay, pl)
        rows[i] = (yuv_image(lay, pl, 4), torch.from_numpy(rgb).cuda())
    for sel in ([0, 1, 2, 3, 4], [5, 4, 3, 2, 0]):
        ims, frames = [rows[i][0] for i in sel], [rows[i][1] for i in sel]
        boxes = [_box((3 * i + 1) % NBOX, im.H, im.W) for i, im in enumerate(ims)]
        _compare(_model(128, 5), ims, frames, boxes, (80, 256), sel)
    sel = [0, 1, 2, 3, 4, 5] * 7
    ims, frames = [rows[i][0] for i in sel], [rows[i][1] for i in sel]
    boxes = [_box(i % NBOX, im.H, im.W) for i, im in enumerate(ims)]
    _compare(_model(128, len(sel)), ims, frames, boxes, (128, 256), sel)


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_contiguous_chw_tensor_of_33_by_35_with_plane1_at_an_odd_address(order):
    import torch
    from vittracker_amd import native
    rs = np.random.RandomState(11)
    B, H, W = 8, 33, 35
    batch = torch.from_numpy(rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)).cuda()
    ims = native.images_from_chw(batch, order)
    assert any(im.planes[1].data_ptr() % 4 for im in ims) and ims[0].planes[0].data_ptr() == batch.data_ptr()
    hwc = batch.permute(0, 2, 3, 1).contiguous()
    frames = [f.clone() if order == "rgb" else f.flip(-1).contiguous() for f in hwc]      # allocations of their own: 4-byte aligned
    boxes = [_box(b % NBOX, H, W) for b in range(B)]
    _compare(_model(128, B), ims, frames, boxes, (64, 80, 256), list(range(B)))
    _compare(_model(128, 1), ims[3:4], frames[3:4], boxes[3:4], (128, 80), [3])


def test_unusable_descriptors_poison_their_own_sequence_only():
    """One unusable descriptor per rule of the header in a table of good ones; each bad descriptor's planes point one past the end of a
    small allocation with extents that would be legal, so a kernel that read through it would read outside it.  T = 64 / 37: general
    kernel, 256: band kernel."""
    import torch
    from vittracker_amd.native import ImageTable
    combos = [op.COMBOS[i % len(op.COMBOS)] for i in range(20)]
    ims = [_case(c, 1)[0] for c in combos]      # 64 x 48 each
    H, W = 64, 48
    B = len(ims)
    mdl = _model(128, B)
    boxes = torch.tensor([_box(8, H, W)] * B, dtype=torch.float64).cuda()
    good = ImageTable.of(ims)
    bad = ImageTable(B, "cuda")
    for i, im in enumerate(ims):
        bad.set_image(i, im)
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    end = small.data_ptr() + small.numel()
    poison = {}

    def spoil(i, **kw):
        d = dict(zip(bad.DTYPE.names, bad.host[i].tolist()))
        d.update(plane0=end, plane1=end, pitch0=0, pitch1=0)
        d.update(kw)
        bad.set(i, tuple(d[n] for n in bad.DTYPE.names), check=False)
        poison[i] = kw

    lay = lambda i: combos[i][0]      # noqa: E731
    assert [lay(i) for i in (0, 1, 2, 6)] == ["rgbp", "bgrp", "i444", "i422"]
    spoil(0, format=16 | 1 << 8)                                # a matrix on RGBP
    spoil(1, format=17 | 1 << 12)                               # a range on BGRP
    spoil(2, plane0=0)                                          # I444 without luma
    spoil(6, W=W - 1)                                           # I422 odd W
    spoil(7, plane1=0)                                          # I422 without chroma
    spoil(8, pitch0=W - 1)                                      # I422 short luma pitch
    spoil(9, pitch1=W // 2 - 1)                                 # I422 short chroma pitch
    spoil(10, pitch1=W - 1)                                     # RGBP short pitch of the trailing planes
    spoil(11, pitch1=1 << 26)                                   # BGRP: 2 H - 1 = 127 rows of 2^26 bytes do not fit 32 bits (63 would)
    spoil(12, format=14)                                        # never assigned
    spoil(13, format=15)
    spoil(14, format=20)                                        # beyond the last layout
    spoil(15, reserved=1)
    spoil(16, format=18 | 2 << 8)                               # matrix 2 on I444
    spoil(17, format=19 | 1 << 16)                              # a bit in 16-31
    spoil(18, pitch0=1 << 32)                                   # a pitch beyond 32 bits
    assert int(bad.host[11]["pitch1"]) * (H - 1) + W <= 0xfffffff0 < int(bad.host[11]["pitch1"]) * (2 * H - 1) + W
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
                assert not np.isnan(float(r8[b])) and int(p8[b].to(torch.int64).sum()) > 0


def _chw_steps(rs, n, B, H, W):
    """n batches (B, 3, H, W) on the device and, per batch, its frames as tight HWC tensors (allocations of their own: a vt_frame wants
    4-byte alignment, which frame b of an odd-sized batch does not have)."""
    import torch
    chw = [torch.from_numpy(rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)).cuda() for _ in range(n)]
    return chw, [[f.clone() for f in c.permute(0, 2, 3, 1).contiguous()] for c in chw]


def _run_steps(mdl, geom, B, box0, n, tables, images):
    """n tracker steps from box0 on tables[t] (ImageTable or FrameTable): records and states after every step."""
    import torch
    from vittracker_amd.native import Outputs
    x = torch.empty(B, 3, geom, geom, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, geom // 16, "cuda")
    st = box0.clone()
    recs, states = [], []
    for t in range(n):
        rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
        step = mdl.track_step_images if images else mdl.track_step_frames
        step(tables[t], st, 4.0, MEAN, STD, x, rf, out, record=rec)
        recs.append(rec)
        states.append(st.clone())
    return torch.stack(recs), torch.stack(states)


@pytest.mark.parametrize("open_loop", [False, True], ids=["free-running", "open-loop"])
def test_step_on_chw_frames_equals_the_frame_step(open_loop):
    """vt_track_step_images on images_from_chw frames == vt_track_step_frames on the permuted frames: G128, B = 4, three steps."""
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import FrameTable, ImageTable
    geom, B, n = 128, 4, 3
    rs = np.random.RandomState(21)
    chw, hwc = _chw_steps(rs, n, B, 97, 131)
    mdl = _model(geom, B)
    mdl.set_template(torch.from_numpy(rs.standard_normal((B, 3, geom // 2, geom // 2)).astype(np.float32)).cuda())
    mdl.set_open_loop(open_loop)
    box0 = torch.tensor([[40.0, 30.0, 30.0, 22.0], [100.0, 70.0, 25.0, 20.0], [2.0, 3.0, 18.0, 14.0], [60.0, 50.0, 12.0, 30.0]],
                        dtype=torch.float64).cuda()
    want = _run_steps(mdl, geom, B, box0, n, [FrameTable.of(f) for f in hwc], False)
    got = _run_steps(mdl, geom, B, box0, n, [ImageTable.of(native.images_from_chw(c)) for c in chw], True)
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(want[1][-1], box0) == open_loop


def test_vit_family_step_on_chw_frames_equals_the_frame_step():
    """The uint8-patch route of a small family="vit" model (width 192, 3 heads, depth 2, 128 / 256, B = 2), one step."""
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import FrameTable, ImageTable
    from vit_small_cases import sd_of
    B, TZ, TX = 2, 128, 256
    mdl = native.Model(TZ, TX, channels=192, heads=3, depth=2, head_channels=256, max_batch=B, family="vit")
    mdl.load_state_dict(sd_of("vitt", "256", 2, 26))
    assert mdl.patch_u8_supported(B)
    rs = np.random.RandomState(23)
    chw, hwc = _chw_steps(rs, 2, B, 97, 131)
    box0 = torch.tensor([[40.0, 30.0, 30.0, 22.0], [90.0, 60.0, 25.0, 28.0]], dtype=torch.float64).cuda()
    z, _ = mdl.crop_images(ImageTable.of(native.images_from_chw(chw[0])), box0, 2.0, TZ, MEAN, STD)
    zf, _ = mdl.crop_frames(FrameTable.of(hwc[0]), box0, 2.0, TZ, MEAN, STD)
    assert torch.equal(z, zf)
    mdl.set_template(z)
    want = _run_steps(mdl, TX, B, box0, 1, [FrameTable.of(hwc[1])], False)
    got = _run_steps(mdl, TX, B, box0, 1, [ImageTable.of(native.images_from_chw(chw[1]))], True)
    assert bool(torch.isfinite(want[0]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    mdl.close()


def test_captured_step_replays_over_a_table_rewritten_from_rgb_to_rgbp_to_i444():
    import torch
    from vittracker_amd import native
    from vittracker_amd.native import FrameTable, Image, ImageTable, Outputs
    geom, B = 128, 4
    rs = np.random.RandomState(25)
    chw, hwc = _chw_steps(rs, 2, B, 97, 131)
    i444 = [_case(("i444", "bt709", "limited"), k % 3) for k in range(B)]
    rows = [([Image.rgb(f) for f in hwc[0]], hwc[0]), (native.images_from_chw(chw[1]), hwc[1]), ([c[0] for c in i444], [c[1] for c in i444])]
    mdl = _model(geom, B)
    mdl.set_template(torch.from_numpy(rs.standard_normal((B, 3, geom // 2, geom // 2)).astype(np.float32)).cuda())
    box0 = torch.tensor([[10.0, 8.0, 14.0, 12.0], [20.0, 15.0, 12.0, 10.0], [2.0, 3.0, 18.0, 14.0], [12.0, 9.0, 10.0, 16.0]],
                        dtype=torch.float64).cuda()
    want = _run_steps(mdl, geom, B, box0, 3, [FrameTable.of(r[1]) for r in rows], False)
    x, rf, out = torch.empty(B, 3, geom, geom, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda"), Outputs(B, geom // 16, "cuda")
    st, rec = box0.clone(), torch.empty(B, 5, dtype=torch.float64, device="cuda")
    itab = ImageTable(B, "cuda")
    for b in range(B):
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
        for b in range(B):
            itab.set_image(b, ims[b])        # the same table address, other formats, pointers and sizes
        itab.upload()
        g.replay()
        got.append(rec.clone())
    assert torch.equal(torch.stack(got), want[0]) and torch.equal(st, want[1][-1])


def test_batched_tracker_on_images_from_chw_equals_it_on_the_permuted_tensor():
    """initialize / track / reinitialize with images_from_chw(cuda tensor) against the same calls on permute(0, 2, 3, 1).contiguous()."""
    import torch
    from vittracker_amd import native
    from vittracker_amd.batched import BatchedVitTracker
    p = _params("vit_48_h32_g128")
    B, n = 4, 3
    rs = np.random.RandomState(27)
    chw, _ = _chw_steps(rs, n + 2, B, 97, 131)
    boxes = [[40.0, 30.0, 30.0, 22.0], [100.0, 70.0, 25.0, 20.0], [2.0, 3.0, 18.0, 14.0], [60.0, 50.0, 12.0, 30.0]]
    new_box = [10.0, 12.0, 20.0, 16.0]

    def run(planar):
        fr = (lambda c: native.images_from_chw(c)) if planar else (lambda c: c.permute(0, 2, 3, 1).contiguous())
        bt = BatchedVitTracker(p, B)
        bt.initialize(fr(chw[0]), boxes)
        res = []
        for t in range(1, n + 2):
            if t == n:
                one = chw[n + 1][1:2]
                bt.reinitialize([2], native.images_from_chw(one) if planar else [one.permute(0, 2, 3, 1).contiguous()[0]], [new_box])
            r = bt.track(fr(chw[t]), sync=True)
            res.append(np.concatenate([np.asarray(r["target_bbox"], dtype=np.float64), np.asarray(r["confidence"], dtype=np.float64)[:, None]], axis=1))
        return np.stack(res)

    want = run(False)
    assert np.isfinite(want).all() and np.array_equal(run(True), want)
    with pytest.raises(ValueError, match="images_from_chw"):
        BatchedVitTracker(p, B).initialize(chw[0], boxes)      # nothing guesses a layout from a shape


def test_plugin_on_chw_host_arrays_equals_it_on_the_hwc_arrays():
    from vittracker_amd.native import Image
    from vittracker_amd.tracker.vit_dist import get_tracker_class
    p = _params("vit_48_h32_noKD")
    rs = np.random.RandomState(29)
    frames = rs.randint(0, 256, (4, 97, 131, 3)).astype(np.uint8)
    box = {"init_bbox": [40.0, 30.0, 30.0, 24.0]}
    a, b = get_tracker_class()(p, "synthetic"), get_tracker_class()(p, "synthetic")
    a.initialize(frames[0], box)
    b.initialize(Image.chw(np.ascontiguousarray(frames[0].transpose(2, 0, 1))), box)
    for f in frames[1:]:
        assert a.track(f) == b.track(Image.chw(np.ascontiguousarray(f.transpose(2, 0, 1))))
