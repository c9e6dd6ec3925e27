"""GPU: frames in other pixel formats (vt_crop_images, vt_crop_u8_images, vt_track_step_images; native.Image / ImageTable) -- each held
bit for bit to what the *_frames entry points compute on a tight RGB frame holding rgb(d), the numpy oracle's conversion
(tests/pixel_oracle.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from pixel_oracle import FORMATS, random_planes, rgb_of

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# even sizes (NV12 / NV21), narrow planes (the kernels' guarded windows) and one frame larger than the crops
SIZES = [(36, 54), (6, 4), (40, 6), (200, 302), (64, 64), (10, 12), (128, 128), (34, 2)]
PITCH = [0, 3, 0, 8, 0, 0, 5, 0]       # extra bytes per row of every plane (odd: rows at unaligned offsets)


def _model(geom, B, seed=0):
    from vittracker_amd import native, synth
    m = native.Model(geom // 2, geom, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(seed, len_z=(geom // 32) ** 2, len_x=(geom // 16) ** 2))
    return m


def _dev_plane(a, extra):
    """A device copy of host plane `a` in an allocation of its own that ENDS at the plane's last byte, rows `extra` bytes apart beyond
    the row's bytes."""
    import torch
    rows = a.shape[0]
    rb = int(np.prod(a.shape[1:]))
    pitch = rb + extra
    flat = torch.zeros(pitch * (rows - 1) + rb, dtype=torch.uint8, device="cuda")
    v = torch.as_strided(flat, a.shape, (pitch,) + tuple(int(s) for s in np.ascontiguousarray(a).strides[1:]))
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v, flat


def _image(fmt, planes, extra):
    from vittracker_amd.native import Image
    dev = [_dev_plane(a, extra)[0] for a in planes]
    return getattr(Image, fmt)(*dev)


def _boxes(rs, sizes):
    bx = []
    for k, (H, W) in enumerate(sizes):
        if k % 3 == 0:
            bx.append([W - 2.5, H - 2.5, 6.0, 5.0])                        # half outside (bottom-right)
        elif k % 3 == 1:
            bx.append([-3.0, -2.0, max(2.0, W / 2), max(2.0, H / 2)])      # half outside (top-left)
        else:
            bx.append([rs.uniform(0, W), rs.uniform(0, H), rs.uniform(1, 40), rs.uniform(1, 40)])
    return bx


def _case(rs, fmts):
    """Per entry of SIZES (cycled over fmts): (format, host planes, device Image, oracle RGB frame on the device)."""
    import torch
    out = []
    for k, (fmt, (H, W)) in enumerate(zip(fmts, SIZES * ((len(fmts) + len(SIZES) - 1) // len(SIZES)))):
        planes = random_planes(rs, fmt, H, W)
        out.append((fmt, planes, _image(fmt, planes, PITCH[k % len(PITCH)]), torch.from_numpy(rgb_of(fmt, planes)).cuda()))
    return out


def _check_crops(seed, fmts, crop_sizes=(64, 96, 128, 256)):
    import torch
    from vittracker_amd.native import FrameTable, ImageTable
    rs = np.random.RandomState(seed)
    case = _case(rs, fmts)
    B = len(case)
    m = _model(128, B)
    itab = ImageTable.of([c[2] for c in case])
    ftab = FrameTable.of([c[3] for c in case])
    st = torch.tensor(_boxes(rs, [c[2].shape[:2] for c in case]), dtype=torch.float64).cuda()
    for T in crop_sizes:
        p8, r8 = m.crop_u8_images(itab, st, 2.0, T)
        q8, s8 = m.crop_u8_frames(ftab, st, 2.0, T)
        pf, rf = m.crop_images(itab, st, 2.0, T, MEAN, STD)
        qf, sf = m.crop_frames(ftab, st, 2.0, T, MEAN, STD)
        for b in range(B):
            what = (T, b, case[b][0], case[b][2].shape)
            assert torch.equal(p8[b], q8[b]) and float(r8[b]) == float(s8[b]), what
            assert torch.equal(pf[b].view(torch.int32), qf[b].view(torch.int32)) and float(rf[b]) == float(sf[b]), what


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_crops_like_its_rgb_frame(fmt):
    """Band sizes (64 / 128 / 256) and a generic one (96), both outputs; at B = 8 the band sizes run the generic kernel too, the
    child-process test below forces the band kernel."""
    _check_crops(10 + FORMATS.index(fmt), [fmt] * len(SIZES))


def test_a_table_mixing_all_formats_crops_each_frame_alone():
    _check_crops(20, [FORMATS[k % 6] for k in range(36)])       # B = 36: the band kernel at T = 128 and 256


@pytest.mark.parametrize("env", [{"VT_CROP_BAND": "-4"}, {"VT_CROP_BAND": "-2"}])
def test_band_forms_crop_like_the_rgb_frames(env):
    """crop_band_image_kernel at every band size and items per thread, forced in a child (a process reads the switches once)."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_frame_formats as T
T._check_crops(30, [T.FORMATS[k %% 6] for k in range(48)], (64, 128, 256))
print("FORM-OK")
""" % (REPO, os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FORM-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_unusable_descriptors_poison_their_own_sequence_only():
    import torch
    from vittracker_amd.native import ImageTable
    rs = np.random.RandomState(3)
    fmts = ["nv12", "rgb", "bgra", "nv21", "bgr", "rgba"] * 3
    ims = [_image(f, random_planes(rs, f, 40, 50), 0) for f in fmts]
    B = len(ims)
    m = _model(128, B)
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

    spoil(0, format=6)
    spoil(1, reserved=1)
    spoil(2, plane0=0)
    spoil(3, plane1=0)                                          # NV21 without chroma
    spoil(4, plane0=int(bad.host[4]["plane0"]) + 2)
    spoil(6, plane1=int(bad.host[6]["plane1"]) + 1)             # NV12 chroma misaligned
    spoil(7, pitch0=149)                                        # RGB, 3 W = 150
    spoil(8, pitch0=199)                                        # BGRA, 4 W = 200
    spoil(9, pitch1=49)                                         # NV21 chroma
    spoil(12, H=39)                                             # NV12 odd H
    spoil(15, W=49)                                             # NV21 odd W
    spoil(13, H=1 << 21, pitch0=1 << 12)                        # RGB beyond 32-bit offsets: 4096 (2^21 - 1) + 150 > 2^32 - 16
    spoil(16, H=0)
    bad.upload()
    for T in (64, 96, 128, 256):
        ref8, rr8 = m.crop_u8_images(good, boxes, 2.0, T)
        reff, rrf = m.crop_images(good, boxes, 2.0, T, MEAN, STD)
        p8, r8 = m.crop_u8_images(bad, boxes, 2.0, T)
        pf, rf = m.crop_images(bad, boxes, 2.0, T, MEAN, STD)
        for b in range(B):
            if b in poison:
                assert np.isnan(float(r8[b])) and np.isnan(float(rf[b])), (T, b, poison[b])
                assert int(p8[b].abs().sum()) == 0 and bool(torch.isnan(pf[b]).all()), (T, b, poison[b])
            else:
                assert torch.equal(p8[b], ref8[b]) and float(r8[b]) == float(rr8[b]) and torch.equal(pf[b], reff[b]), (T, b)


def _step_frames(rs, B, n, fmts_of):
    """n steps of B frames: per step, per sequence an Image in format fmts_of(step, b) and its oracle RGB frame (device)."""
    import torch
    sizes = [(96, 128), (150, 212), (72, 100), (60, 40)]
    steps = []
    for t in range(n):
        row = []
        for b in range(B):
            H, W = sizes[b % len(sizes)]
            f = fmts_of(t, b)
            planes = random_planes(rs, f, H, W)
            row.append((_image(f, planes, 4 * (b % 2)), torch.from_numpy(rgb_of(f, planes)).cuda()))
        steps.append(row)
    return steps


@pytest.mark.parametrize("geom,B", [(128, 1), (128, 7), (128, 256), (256, 1), (256, 7), (256, 256)])
def test_image_step_equals_the_frame_step(geom, B):
    """vt_track_step_images records and states == vt_track_step_frames on the oracle's RGB frames, closed loop over 8 steps; at B = 7
    also a step captured once and replayed after the table was rewritten with other formats."""
    import torch
    from vittracker_amd.native import FrameTable, ImageTable, Outputs
    n = 8
    rs = np.random.RandomState(40 + B)
    steps = _step_frames(rs, B, n, lambda t, b: FORMATS[(t + b) % 6])
    m = _model(geom, B)
    z = torch.from_numpy(rs.standard_normal((B, 3, geom // 2, geom // 2)).astype(np.float32)).cuda()
    m.set_template(z)
    box0 = torch.tensor([[rs.uniform(0, 30), rs.uniform(0, 20), rs.uniform(10, 30), rs.uniform(10, 25)] for _ in range(B)],
                        dtype=torch.float64).cuda()
    box0[0] = torch.tensor([120.0, 90.0, 30.0, 20.0], dtype=torch.float64)       # clipped at its frame's edge
    x = torch.empty(B, 3, geom, geom, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, geom // 16, "cuda")
    ftab, itab = FrameTable(B, "cuda"), ImageTable(B, "cuda")

    def run(images):
        st = box0.clone()
        recs, states = [], []
        for t in range(n):
            rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
            if images:
                for b in range(B):
                    itab.set_image(b, steps[t][b][0])
                itab.upload()
                m.track_step_images(itab, st, 4.0, MEAN, STD, x, rf, out, record=rec)
            else:
                for b in range(B):
                    ftab.set_tensor(b, steps[t][b][1])
                ftab.upload()
                m.track_step_frames(ftab, st, 4.0, MEAN, STD, x, rf, out, record=rec)
            recs.append(rec)
            states.append(st.clone())
        return torch.stack(recs), torch.stack(states)

    want = run(False)
    got = run(True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if B != 7:
        return
    st = box0.clone()
    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    for b in range(B):
        itab.set_image(b, steps[0][b][0])
    itab.upload()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        m.track_step_images(itab, st, 4.0, MEAN, STD, x, rf, out, record=rec, stream=torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(side)
    st.copy_(box0)
    got = []
    for t in range(n):
        for b in range(B):
            itab.set_image(b, steps[t][b][0])        # every step rewrites the table with other formats and sizes
        itab.upload()
        g.replay()
        got.append(rec.clone())
    assert torch.equal(torch.stack(got), want[0])


def _params(yaml_name):
    from vittracker_amd.parameter import vit_dist as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(yaml_name)
    p.allow_synthetic_weights = True
    p.debug = 0
    return p


def test_batched_tracker_on_nv12_equals_it_on_the_rgb_frames():
    """Device NV12 planes and host NV12 arrays (the pinned arena) give the records of the converted RGB frames, and reinitialize()
    takes an Image."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    p = _params("vit_48_h32_g128")
    B, n = 5, 6
    rs = np.random.RandomState(50)
    sizes = [(240, 320), (120, 160), (72, 100), (40, 6), (130, 96)]
    seq = []
    for t in range(n + 1):
        row = []
        for b in range(B):
            H, W = sizes[b]
            y, uv = random_planes(rs, "nv12", H, W)
            row.append((y, uv, rgb_of("nv12", [y, uv])))
        seq.append(row)
    boxes = [[W * 0.3, H * 0.3, max(2.0, W * 0.2), max(2.0, H * 0.2)] for H, W in sizes]
    boxes[1] = [150.0, 110.0, 14.0, 9.0]             # clipped at its frame's edge
    new_box = [10.0, 12.0, 20.0, 16.0]

    def run(kind):
        def frame(t, b):
            y, uv, rgb = seq[t][b]
            if kind == "rgb":
                return rgb
            if kind == "host":
                return Image.nv12(y, uv)
            return Image.nv12(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda())
        bt = BatchedVitTracker(p, B)
        bt.initialize([frame(0, b) for b in range(B)], boxes)
        recs = [bt.track_record([frame(t, b) for b in range(B)]) for t in range(1, n)]
        bt.reinitialize([2], [frame(n, 0)], [new_box])
        recs.append(bt.track_record([frame(n, b) for b in range(B)]))
        return np.stack(recs)

    want = run("rgb")
    assert np.array_equal(run("dev"), want)
    assert np.array_equal(run("host"), want)


def test_plugin_on_a_bgr_image_equals_it_on_the_rgb_frame():
    from vittracker_amd.native import Image
    from vittracker_amd.tracker.vit_dist import get_tracker_class
    p = _params("vit_48_h32_noKD")
    rs = np.random.RandomState(60)
    frames = rs.randint(0, 256, (5, 150, 206, 3)).astype(np.uint8)
    box = {"init_bbox": [60.0, 40.0, 30.0, 24.0]}
    a, b = get_tracker_class()(p, "synthetic"), get_tracker_class()(p, "synthetic")
    a.initialize(frames[0], box)
    b.initialize(Image.bgr(frames[0][..., ::-1].copy()), box)
    for f in frames[1:]:
        ra, rb = a.track(f), b.track(Image.bgr(f[..., ::-1].copy()))
        assert ra == rb


def test_nv_conversion_matches_opencv():
    """The fixed-point constants were written down from OpenCV's color_yuv.simd.hpp: pinned against cv2.cvtColor where it imports."""
    try:
        import cv2
    except ImportError:
        pytest.skip("cv2 is not installed: the BT.601 constants are not pinned against OpenCV on this machine")
    import torch
    from vittracker_amd.native import FrameTable, ImageTable
    rs = np.random.RandomState(70)
    H, W = 64, 96
    ims, frames = [], []
    for fmt, code in (("nv12", cv2.COLOR_YUV2RGB_NV12), ("nv21", cv2.COLOR_YUV2RGB_NV21)):
        y, c = random_planes(rs, fmt, H, W)
        want = cv2.cvtColor(np.concatenate([y, c.reshape(H // 2, W)], axis=0), code)
        assert np.array_equal(rgb_of(fmt, [y, c]), want), fmt
        ims.append(_image(fmt, [y, c], 0))
        frames.append(torch.from_numpy(want).cuda())
    m = _model(128, 2)
    st = torch.tensor([[10.0, 8.0, 40.0, 30.0]] * 2, dtype=torch.float64).cuda()
    p, _ = m.crop_u8_images(ImageTable.of(ims), st, 1.0, 64)
    q, _ = m.crop_u8_frames(FrameTable.of(frames), st, 1.0, 64)
    assert torch.equal(p, q)
