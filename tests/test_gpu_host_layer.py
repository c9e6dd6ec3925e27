"""GPU: the edges of the Python host layer that every route shares -- the pinned arenas of BatchedVitTracker growing between two steps,
a pinned descriptor table rewritten while its upload is still queued, and hold_states() dropping every route's captured steps.  All at
G128 with synthetic weights; every comparison is bit for bit."""
import numpy as np
import pytest

from pixel_oracle import random_planes, rgb_of
from test_gpu_frame_formats import _image
from test_gpu_frame_table import _model, _params, _solo

pytestmark = pytest.mark.gpu

SMALL = [(40, 56), (33, 47), (64, 64)]
EVEN = [(40, 56), (34, 48), (64, 64)]             # the image route's: NV12 wants even sizes


def _steps(small):
    """Per step after initialize(): the frame sizes of the three sequences.  Step 3 is beyond twice the first capacity (the arena
    grows to exactly `end`), step 4 lies within the grown arena (no growth), step 5 is small again."""
    return [small, small, [(300, 400)] + small[1:], [small[0], (120, 160), small[2]], small]


def _box(H, W):
    return [W * 0.3, H * 0.3, max(2.0, W * 0.2), max(2.0, H * 0.2)]


def test_growth_steps_are_what_they_claim():
    """The sizes above against the packers: growth at step 3 only, to `end` (not to twice the capacity)."""
    from vittracker_amd.native import FrameTable, ImageTable, pack_offsets, pack_planes
    nv12 = lambda H, W: [H * W, H * W // 2]
    for ends in ([pack_offsets(s, start=3 * FrameTable.ITEM)[1] for s in [SMALL] + _steps(SMALL)],
                 [pack_planes([nv12(*s[0]), [s[1][0] * s[1][1] * 3]], 3 * ImageTable.ITEM)[1] for s in [EVEN] + _steps(EVEN)]):
        assert ends[3] > 2 * ends[0] and max(ends[:3]) == ends[0] and ends[4] <= ends[3] and ends[5] == ends[0]


def test_frame_arena_growth_between_steps_keeps_every_sequence_on_its_own_frames():
    from vittracker_amd.batched import BatchedVitTracker
    p = _params("vit_48_h32_g128")
    rs = np.random.RandomState(80)
    seqs = [[rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes] for sizes in zip(SMALL, *_steps(SMALL))]
    boxes = [_box(*s) for s in SMALL]
    bt = BatchedVitTracker(p, 3)
    bt.initialize([s[0] for s in seqs], boxes)
    recs = np.stack([bt.track_record([s[t] for s in seqs]) for t in range(1, len(seqs[0]))])
    for b in range(3):
        assert np.array_equal(recs[:, b], _solo(p, 3, seqs[b], boxes[b])), b


def test_image_arena_growth_between_steps_equals_the_tracker_on_the_rgb_frames():
    """Sequence 0 host NV12 (it forces the growth), sequence 1 a host RGB array, sequence 2 a device BGR Image read in place."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    p = _params("vit_48_h32_g128")
    rs = np.random.RandomState(81)
    fmts = ("nv12", "rgb", "bgr")
    planes = [[random_planes(rs, f, H, W) for f, (H, W) in zip(fmts, sizes)] for sizes in [EVEN] + _steps(EVEN)]
    boxes = [_box(*s) for s in EVEN]

    def frames(t, images):
        pl = planes[t]
        if not images:
            return [rgb_of(f, q) for f, q in zip(fmts, pl)]
        return [Image.nv12(*pl[0]), pl[1][0], Image.bgr(torch.from_numpy(pl[2][0]).cuda())]

    def run(images):
        bt = BatchedVitTracker(p, 3)
        bt.initialize(frames(0, images), boxes)
        return np.stack([bt.track_record(frames(t, images)) for t in range(1, len(planes))])

    assert np.array_equal(run(True), run(False))


def test_a_pinned_table_rewritten_while_its_upload_is_queued():
    """upload() queues the copy out of the pinned host table; set_tensor / set_image right behind it must wait for that copy before
    the CPU writes, and the second upload must carry the new entries: each patch is that entry's frame cropped alone."""
    import torch
    from vittracker_amd.native import FrameTable, Image, ImageTable
    rs = np.random.RandomState(82)
    sizes = [(40, 56), (34, 48), (64, 64), (20, 90), (50, 30), (72, 100)]
    rgb = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    dev = [torch.from_numpy(a).cuda() for a in rgb]
    fmts = ("nv12", "bgr", "rgb", "bgra", "nv21", "rgba")
    planes = [random_planes(rs, f, H, W) for f, (H, W) in zip(fmts, sizes)]
    ims = [_image(f, q, 0) for f, q in zip(fmts, planes)]
    m = _model(128, 4)
    st = torch.tensor([_box(H, W) for H, W in sizes], dtype=torch.float64).cuda()
    final = [0, 4, 2, 5]                       # entries 1 and 3 are rewritten behind the first upload
    stf = st[final].contiguous()

    def alone(frame, b):
        return m.crop_u8(torch.from_numpy(np.ascontiguousarray(frame)[None]).cuda(), stf[b:b + 1].contiguous(), 2.0, 128)[0][0]

    ft = FrameTable(4, "cuda")
    for i in range(4):
        ft.set_tensor(i, dev[i])
    ft.upload()
    ft.set_tensor(1, dev[4])
    ft.set_tensor(3, dev[5])
    ft.upload()
    got, _ = m.crop_u8_frames(ft, stf, 2.0, 128)
    for b, k in enumerate(final):
        assert torch.equal(got[b], alone(rgb[k], b)), ("frames", b)

    it = ImageTable(4, "cuda")
    for i in range(4):
        it.set_image(i, ims[i])
    it.upload()
    it.set_image(1, ims[4])
    it.set_image(3, ims[5])
    it.upload()
    got, _ = m.crop_u8_images(it, stf, 2.0, 128)
    for b, k in enumerate(final):
        assert torch.equal(got[b], alone(rgb_of(fmts[k], planes[k]), b)), ("images", b)


def test_hold_states_drops_the_captured_steps_of_every_route():
    """Steps on the dense, the mixed and the image route capture closed-loop graphs; hold_states(True) must drop all of them: the next
    step of each route leaves `states` alone and gives the records of a fresh tracker held at the same boxes."""
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import Image
    p = _params("vit_48_h32_g128")
    rs = np.random.RandomState(83)
    dense = rs.randint(0, 256, (3, 3, 96, 128, 3)).astype(np.uint8)
    mixed = [[rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in SMALL] for _ in range(2)]
    nv = [[random_planes(rs, "nv12", H, W) for H, W in EVEN] for _ in range(2)]
    boxes = [_box(96, 128)] * 3

    def routes(bt, t):
        return np.stack([bt.track_record(dense[1 + t]), bt.track_record(mixed[t]), bt.track_record([Image.nv12(*q) for q in nv[t]])])

    bt = BatchedVitTracker(p, 3)
    bt.initialize(dense[0], boxes)
    routes(bt, 0)
    held = bt.states.clone()
    bt.hold_states(True)
    got = routes(bt, 1)
    assert bool((bt.states == held).all())
    fresh = BatchedVitTracker(p, 3)
    fresh.initialize(dense[0], boxes)
    fresh.states.copy_(held)
    fresh.hold_states(True)
    assert np.array_equal(got, routes(fresh, 1))
