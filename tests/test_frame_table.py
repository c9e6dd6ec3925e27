"""CPU: the host side of batches of mixed frame sizes -- FrameTable packing and checks, the continuous-batching runner
(run_dataset_continuous) driven by a fake batched tracker that records its calls, and the synthetic_mixed dataset."""
import os
import types

import numpy as np
import pytest

from vittracker_amd.native import ARENA_ALIGN, FRAME_DTYPE, FrameTable, VtError, pack_offsets


def test_frame_descriptor_matches_the_c_struct():
    assert FRAME_DTYPE.itemsize == 24
    assert [FRAME_DTYPE.fields[k][1] for k in ("data", "H", "W", "pitch")] == [0, 8, 12, 16]


def test_pack_offsets_are_aligned_and_disjoint():
    shapes = [(240, 320), (201, 301), (40, 5), (1, 1), (72, 100)]
    offs, end = pack_offsets(shapes, start=24 * 5)
    assert all(o % ARENA_ALIGN == 0 for o in offs) and offs[0] >= 24 * 5
    for (o, (H, W)), o2 in zip(zip(offs, shapes), offs[1:] + [end]):
        assert o + H * W * 3 <= o2
    assert end == offs[-1] + 72 * 100 * 3


def test_one_packer_serves_frames_and_image_planes():
    """pack_planes against offsets written down from pack_offsets / pack_image_offsets as they were before they shared it: odd widths,
    a 1 x 1 frame, two-plane images, a start behind a table and an alignment other than the arena's."""
    from vittracker_amd.native import Image, pack_image_offsets, pack_planes
    shapes = [(1, 1), (33, 47), (40, 5), (201, 301), (64, 64), (7, 3)]
    want = {(24 * 6, 256): ([256, 512, 5376, 6144, 187648, 199936], 199999),
            (0, 256): ([0, 256, 5120, 5888, 187392, 199680], 199743),
            (100, 4): ([100, 104, 4760, 5360, 186864, 199152], 199215)}
    for (start, align), (offs, end) in want.items():
        assert pack_offsets(shapes, start=start, align=align) == (offs, end)
        assert pack_planes([[H * W * 3] for H, W in shapes], start, align) == ([[o] for o in offs], end)
    z = lambda *s: np.zeros(s, np.uint8)
    ims = [Image.nv12(z(36, 54), z(18, 27, 2)), Image.rgb(z(1, 1, 3)), Image.i420(z(6, 4), z(3, 2), z(3, 2)), Image.gray(z(5, 7)),
           Image.yuyv(z(3, 6, 2)), Image.p010(np.zeros((10, 12), np.uint16), np.zeros((5, 6, 2), np.uint16)), Image.bgra(z(9, 11, 4)),
           Image.rgb(z(33, 47, 3))]
    want = {(48 * 8, 256): ([[512, 2560], [3584], [3840, 4096], [4352], [4608], [4864, 5120], [5376], [5888]], 10541),
            (0, 256): ([[0, 2048], [3072], [3328, 3584], [3840], [4096], [4352, 4608], [4864], [5376]], 10029),
            (100, 4): ([[100, 2044], [3016], [3020, 3044], [3056], [3092], [3128, 3368], [3488], [3884]], 8537)}
    sizes = [[rows * rb for rows, rb in im.plane_rows()] for im in ims]
    assert sizes == [[1944, 972], [3], [24, 12], [35], [36], [240, 120], [396], [4653]]
    for (start, align), (offs, end) in want.items():
        assert pack_image_offsets(ims, start=start, align=align) == (offs, end)
        assert pack_planes(sizes, start, align) == (offs, end)


def test_frame_table_checks_every_descriptor():
    t = FrameTable(3)
    t.set(0, 4096, 10, 7)                              # pitch 0 -> 3 W
    assert t.host[0]["pitch"] == 21 and t.host[0]["H"] == 10 and t.host[0]["W"] == 7
    t.set(1, 8192, 10, 7, pitch=64, nbytes=64 * 9 + 21)      # a frame exactly filling its buffer, at pitch > 3 W
    assert t.host[1]["pitch"] == 64
    with pytest.raises(VtError, match="aligned"):
        t.set(2, 4098, 10, 7)
    with pytest.raises(VtError, match="shorter than a row"):
        t.set(2, 4096, 10, 7, pitch=20)
    with pytest.raises(VtError, match="needs"):
        t.set(2, 4096, 10, 7, pitch=64, nbytes=64 * 9 + 20)          # one byte short
    with pytest.raises(VtError, match=">= 1"):
        t.set(2, 4096, 0, 7)
    with pytest.raises(VtError):
        t.set(2, 0, 10, 7)


def test_frame_table_from_tensors_takes_strided_rows_but_not_strided_pixels():
    import torch
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    t = FrameTable(2)
    t.set_tensor(0, img[4:20, 8:40], device_only=False)       # a window of a larger image: pitch = 3 x 80
    assert (t.host[0]["H"], t.host[0]["W"], t.host[0]["pitch"]) == (16, 32, 240)
    assert t.host[0]["data"] == img[4:20, 8:40].data_ptr()
    with pytest.raises(VtError, match="strides"):
        t.set_tensor(1, img[:, ::2], device_only=False)
    with pytest.raises(VtError, match="uint8"):
        t.set_tensor(1, img.float(), device_only=False)
    with pytest.raises(VtError, match="GPU or in pinned"):
        t.set_tensor(1, img)


def test_synthetic_mixed_is_deterministic_and_mixed():
    from vittracker_amd.evaluation import get_dataset
    a, b = get_dataset("synthetic_mixed:10x6"), get_dataset("synthetic_mixed:10x6")
    assert [s.name for s in a] == [s.name for s in b]
    for s, t in zip(a, b):
        assert len(s) == len(t) and np.array_equal(s.ground_truth_rect, t.ground_truth_rect)
        assert all(np.array_equal(f, g) for f, g in zip(s.frames, t.frames))
    sizes = {s.frames[0].shape[:2] for s in a}
    assert len(sizes) >= 4
    assert any((3 * w) % 4 for _, w in sizes) and any(w < 6 or h < 128 for h, w in sizes)
    assert all(6 <= len(s) <= 12 for s in a) and len({len(s) for s in a}) > 2
    for s in a:
        H, W = s.frames[0].shape[:2]
        x, y, w, h = s.ground_truth_rect[0]
        assert 0 <= x and x + w <= W and 0 <= y and y + h <= H and w >= 2 and h >= 2
    # the plain synthetic spec is unchanged
    assert len(get_dataset("synthetic:3x4")) == 3


class _FakeBatched:
    """Records every call; a box is a function of the frame it was computed on and of the slot's history, so that the files
    show whether each sequence saw its own frames in order."""
    log = []

    def __init__(self, params, B):
        self.B = B
        self.state = [None] * B
        _FakeBatched.log.append(("new", B))

    @staticmethod
    def _sig(f):
        return float(np.asarray(f, dtype=np.float64).sum() % 9973)

    def initialize(self, frames, boxes):
        assert len(frames) == self.B and len(boxes) == self.B
        self.state = [list(map(float, b)) for b in boxes]
        _FakeBatched.log.append(("init", [self._sig(f) for f in frames]))

    def reinitialize(self, slots, frames, boxes):
        for b, bx in zip(slots, boxes):
            self.state[b] = list(map(float, bx))
        _FakeBatched.log.append(("reinit", list(slots), [self._sig(f) for f in frames]))

    def track(self, frames):
        import torch
        assert isinstance(frames, list) and len(frames) == self.B
        sig = [self._sig(f) for f in frames]
        for b in range(self.B):
            x, y, w, h = self.state[b]
            self.state[b] = [x + sig[b] % 7, y + 1, w, h]
        _FakeBatched.log.append(("track", sig))
        return {"target_bbox": torch.tensor(self.state, dtype=torch.float64)}


def _tracker(tmp_path):
    os.makedirs(tmp_path, exist_ok=True)
    p = types.SimpleNamespace(template_factor=2.0, search_factor=4.0, debug=0)
    return types.SimpleNamespace(name="fake", parameter_name="p", run_id=None, results_dir=str(tmp_path), get_parameters=lambda: p)


def _read(d, s, suffix=""):
    return open(os.path.join(d, s.name + suffix + ".txt")).read()


def test_continuous_runner_steps_every_sequence_through_its_own_frames(tmp_path):
    from vittracker_amd.evaluation import get_dataset
    from vittracker_amd.evaluation.running import run_dataset_continuous
    ds = get_dataset("synthetic_mixed:10x6")
    _FakeBatched.log = []
    tc = _tracker(tmp_path / "cont")
    out = run_dataset_continuous(ds, tc, batch=4, make_batched=_FakeBatched)
    log = _FakeBatched.log
    assert log[0] == ("new", 4) and sum(1 for e in log if e[0] == "new") == 1
    sig = _FakeBatched._sig
    # which sequence each slot runs, replayed from the log: frame 0 at (re)initialisation, then frames 1.. in order, once each
    slot_seq, slot_t, seen = [None] * 4, [0] * 4, {s.name: [] for s in ds}
    pending = list(ds)
    init = log[1]
    assert init[0] == "init"
    for b in range(4):
        s = pending.pop(0)
        assert init[1][b] == sig(s.frames[0])
        slot_seq[b], slot_t[b] = s, 1
        seen[s.name].append(0)
    finished_at = {}
    step = 0
    for e in log[2:]:
        if e[0] == "reinit":
            for b, g in zip(e[1], e[2]):
                # refilled on the step right after its previous sequence ended
                assert slot_seq[b] is None and finished_at[b] == step
                s = pending.pop(0)
                assert g == sig(s.frames[0])
                slot_seq[b], slot_t[b] = s, 1
                seen[s.name].append(0)
        else:
            step += 1
            for b in range(4):
                s = slot_seq[b]
                if s is None:
                    continue
                assert e[1][b] == sig(s.frames[slot_t[b]])
                seen[s.name].append(slot_t[b])
                slot_t[b] += 1
                if slot_t[b] == len(s):
                    slot_seq[b] = None
                    finished_at[b] = step
    assert not pending
    for s in ds:
        assert seen[s.name] == list(range(len(s))), s.name
        assert len(out[s.name]["target_bbox"]) == len(s) and len(out[s.name]["time"]) == len(s)
    # the files equal a run of each sequence alone
    for s in ds:
        _FakeBatched.log = []
        solo = _tracker(tmp_path / "solo" / s.name)
        run_dataset_continuous([s], solo, batch=1, make_batched=_FakeBatched)
        assert _read(solo.results_dir, s) == _read(tc.results_dir, s), s.name
        tl = _read(tc.results_dir, s, "_time").splitlines()
        assert len(tl) == len(s) and all(float(v) >= 0 for v in tl)


def test_continuous_runner_screens_too_small_boxes_and_shards_by_rank(tmp_path):
    from vittracker_amd.evaluation import get_dataset
    from vittracker_amd.evaluation.running import run_dataset_continuous
    ds = list(get_dataset("synthetic_mixed:6x3"))
    ds[2].ground_truth_rect[0, 2:] = 0.0                   # 'Too small bounding box.': skipped alone
    _FakeBatched.log = []
    out = run_dataset_continuous(ds, _tracker(tmp_path / "a"), batch=8, make_batched=_FakeBatched)
    assert set(out) == {s.name for i, s in enumerate(ds) if i != 2}
    out = run_dataset_continuous(ds, _tracker(tmp_path / "b"), batch=2, rank=1, world=2, make_batched=_FakeBatched)
    assert set(out) == {ds[i].name for i in (1, 3, 5)}


def test_sharded_tracker_refuses_continuous_batching():
    from vittracker_amd.batched import ShardedBatchedTracker
    t = ShardedBatchedTracker.__new__(ShardedBatchedTracker)
    with pytest.raises(VtError, match="ShardedBatchedTracker"):
        t.reinitialize([0], [np.zeros((4, 4, 3), np.uint8)], [[0, 0, 2, 2]])
