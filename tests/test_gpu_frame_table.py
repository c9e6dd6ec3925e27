"""GPU: batches of frames of different sizes (vt_crop_frames, vt_crop_u8_frames, vt_track_step_frames), restarting single slots
(vt_set_template_slots) and the continuous-batching runner -- each held bit for bit to what the dense entry points, solo trackers or the
sequential runner compute."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _model(geom, B, seed=0, search=None):
    from vittracker_amd import native, synth
    S = search or geom
    Tz = S // 2
    m = native.Model(Tz, S, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(seed, len_z=(Tz // 16) ** 2, len_x=(S // 16) ** 2))
    return m


def _mixed_frames(rs, sizes, pitch_extra):
    """Device frames of the given sizes, each in a buffer of its own: extra = 0 fills the buffer exactly (the frame's last byte is the
    allocation's last byte), extra > 0 is a window of a wider image (pitch > 3 W)."""
    import torch
    out, host = [], []
    for (H, W), ex in zip(sizes, pitch_extra):
        if ex == 0:
            a = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
            out.append(torch.from_numpy(a).cuda())
        else:
            big = torch.from_numpy(rs.randint(0, 256, (H, W + ex, 3)).astype(np.uint8)).cuda()
            out.append(big[:, ex:])           # rows at pitch 3 (W + ex), first pixel 3 ex bytes in: ex even keeps 4-byte alignment
            a = out[-1].cpu().numpy()
        host.append(np.ascontiguousarray(a))
    return out, host


SIZES = [(37, 53), (5, 4), (40, 5), (200, 301), (64, 64), (9, 11), (128, 128), (33, 2)]
PITCH = [0, 0, 4, 0, 8, 0, 4, 0]


def _boxes(rs, sizes):
    bx = []
    for k, (H, W) in enumerate(sizes):
        if k % 3 == 0:
            bx.append([W - 2.5, H - 2.5, 6.0, 5.0])                    # half outside the frame (bottom-right)
        elif k % 3 == 1:
            bx.append([-3.0, -2.0, max(2.0, W / 2), max(2.0, H / 2)])      # half outside (top-left)
        else:
            bx.append([rs.uniform(0, W), rs.uniform(0, H), rs.uniform(1, 40), rs.uniform(1, 40)])
    return bx


def _check_crops(sizes, pitch, seed, crop_sizes=(64, 128, 256)):
    import torch
    from vittracker_amd.host_ops import sample_target
    from vittracker_amd.native import FrameTable
    rs = np.random.RandomState(seed)
    dev, host = _mixed_frames(rs, sizes, pitch)
    boxes = _boxes(rs, sizes)
    B = len(sizes)
    m = _model(128, B)
    tab = FrameTable.of(dev)
    st = torch.tensor(boxes, dtype=torch.float64).cuda()
    for T in crop_sizes:
        p8, rf8 = m.crop_u8_frames(tab, st, 2.0, T)
        pf, rff = m.crop_frames(tab, st, 2.0, T, MEAN, STD)
        for b in range(B):
            one = torch.from_numpy(host[b][None]).cuda()
            q8, qr8 = m.crop_u8(one, st[b:b + 1].contiguous(), 2.0, T)
            qf, qrf = m.crop(one, st[b:b + 1].contiguous(), 2.0, T, MEAN, STD)
            assert torch.equal(p8[b], q8[0]) and float(rf8[b]) == float(qr8[0]), (T, b, sizes[b])
            assert torch.equal(pf[b].view(torch.int32), qf[0].view(torch.int32)) and float(rff[b]) == float(qrf[0]), (T, b, sizes[b])
            want, want_rf, _ = sample_target(host[b], list(boxes[b]), 2.0, output_sz=T)
            assert np.array_equal(p8[b].cpu().numpy(), want) and float(rf8[b]) == want_rf, (T, b, sizes[b])


def test_table_crops_equal_each_frame_cropped_alone():
    _check_crops(SIZES, PITCH, 0)


@pytest.mark.parametrize("env", [{"VT_CROP_BYTES": "1"}, {"VT_CROP_FAST": "0"}, {"VT_CROP_BAND": "0"}, {"VT_CROP_BAND": "-4"}, {"VT_CROP_BAND": "-2"},
                                 {"VT_CROP_BAND": "-4", "VT_CROP_ALIGNED": "0"}])
def test_every_table_crop_form_equals_each_frame_cropped_alone(env):
    """Each crop form forced through the environment in a child (a process reads the switches once), as tests/test_gpu_patch_u8.py does."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_frame_table as T
T._check_crops(T.SIZES, T.PITCH, 1)
print("FORM-OK")
""" % (REPO, os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "FORM-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_invalid_descriptors_poison_their_own_sequence_only():
    import torch
    from vittracker_amd.native import FrameTable
    rs = np.random.RandomState(2)
    sizes = [(40, 50)] * 6
    dev, host = _mixed_frames(rs, sizes, [0] * 6)
    m = _model(128, 6)
    boxes = torch.tensor([[5.0, 6.0, 20.0, 15.0]] * 6, dtype=torch.float64).cuda()
    good = FrameTable.of(dev)
    ref8, rr8 = m.crop_u8_frames(good, boxes, 2.0, 128)
    reff, rrf = m.crop_frames(good, boxes, 2.0, 128, MEAN, STD)
    bad = FrameTable(6, "cuda")
    for i, f in enumerate(dev):
        bad.set_tensor(i, f)
    p0 = int(bad.host[1]["data"])
    bad.host[1] = (0, 40, 50, 0)                  # null data
    bad.host[2] = (p0, 0, 50, 0)                  # H < 1
    bad.host[3] = (p0 + 2, 40, 50, 0)             # misaligned
    bad.host[4] = (p0, 40, 50, 149)               # pitch < 3 W
    bad.upload()
    p8, r8 = m.crop_u8_frames(bad, boxes, 2.0, 128)
    pf, rf = m.crop_frames(bad, boxes, 2.0, 128, MEAN, STD)
    for b in range(6):
        if b in (1, 2, 3, 4):
            assert np.isnan(float(r8[b])) and np.isnan(float(rf[b])) and int(p8[b].abs().sum()) == 0 and bool(torch.isnan(pf[b]).all())
        else:
            assert torch.equal(p8[b], ref8[b]) and float(r8[b]) == float(rr8[b]) and torch.equal(pf[b], reff[b])


@pytest.mark.parametrize("geom,search,B", [(128, None, 1), (128, None, 5), (128, None, 256), (256, None, 1), (256, None, 5), (256, None, 256),
                                          (224, 224, 3)])
def test_table_step_equals_the_dense_step(geom, search, B):
    """All frames the same size, the table pointing into one dense buffer: vt_track_step_frames records == vt_track_step records, eager and
    graph-captured, and a graph replayed after the table's contents were rewritten (to a second dense buffer)."""
    import torch
    from vittracker_amd.native import FrameTable, Outputs
    S = search or geom
    m = _model(geom, B, search=search)
    rs = np.random.RandomState(3)
    H, W = 150, 212          # every frame of the dense buffer 4-byte aligned (vt_frame.data must be)
    frames = [torch.from_numpy(rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).cuda() for _ in range(3)]
    box0 = torch.tensor([[rs.uniform(0, W - 40), rs.uniform(0, H - 30), rs.uniform(10, 40), rs.uniform(10, 30)] for _ in range(B)],
                        dtype=torch.float64).cuda()
    box0[0] = torch.tensor([W - 12.0, H - 9.0, 30.0, 20.0], dtype=torch.float64)       # clipped at the frame's edge
    z = torch.from_numpy(rs.standard_normal((B, 3, S // 2, S // 2)).astype(np.float32)).cuda()
    m.set_template(z)
    x = torch.empty(B, 3, S, S, device="cuda")
    rf = torch.empty(B, dtype=torch.float64, device="cuda")
    out = Outputs(B, S // 16, "cuda")

    def dense(n):
        st = box0.clone()
        recs = []
        for i in range(n):
            rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
            m.track_step(frames[i], st, 4.0, MEAN, STD, x, rf, out, record=rec)
            recs.append(rec)
        return torch.stack(recs)

    want = dense(3)
    tab = FrameTable(B, "cuda")

    def point(i):
        for b in range(B):
            tab.set_tensor(b, frames[i][b])
        tab.upload()

    st = box0.clone()
    got = []
    for i in range(3):
        point(i)
        rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
        m.track_step_frames(tab, st, 4.0, MEAN, STD, x, rf, out, record=rec)
        got.append(rec)
    assert torch.equal(torch.stack(got), want)
    # captured once on the table's address, replayed with the table rewritten before each replay
    st.copy_(box0)
    rec = torch.empty(B, 5, dtype=torch.float64, device="cuda")
    point(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        m.track_step_frames(tab, st, 4.0, MEAN, STD, x, rf, out, record=rec, stream=torch.cuda.current_stream())
    torch.cuda.current_stream().wait_stream(side)
    st.copy_(box0)
    got = []
    for i in range(3):
        point(i)
        g.replay()
        got.append(rec.clone())
    assert torch.equal(torch.stack(got), want)


def _params(yaml_name):
    from vittracker_amd.parameter import vit_dist as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(yaml_name)
    p.allow_synthetic_weights = True
    p.debug = 0
    return p


def _mixed_seq(rs, B, T):
    sizes = [(240, 320), (201, 301), (72, 100), (40, 5), (130, 97), (64, 64)]
    seqs = []
    for b in range(B):
        H, W = sizes[b % len(sizes)]
        fr = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(T)]
        if b % 4 == 1:
            box = [max(0.0, W - 6.0), max(0.0, H - 5.0), 12.0, 9.0]        # clipped at its own frame's edge
        else:
            box = [W * 0.3, H * 0.3, max(2.0, W * 0.2), max(2.0, H * 0.2)]
        seqs.append((fr, box))
    return seqs


def _solo(p, B, fr, box):
    from vittracker_amd.batched import BatchedVitTracker
    t = BatchedVitTracker(p, 1, form_batch=B)
    t.initialize(fr[0][None], [box])
    return np.stack([t.track_record(f[None])[0] for f in fr[1:]])


@pytest.mark.parametrize("yaml_name,B", [("vit_48_h32_g128", 6), ("vit_48_h32_noKD", 6), ("vit_48_h32_g128", 256)])
def test_mixed_closed_loop_equals_solo_trackers(yaml_name, B):
    from vittracker_amd.batched import BatchedVitTracker
    p = _params(yaml_name)
    rs = np.random.RandomState(4)
    T = 10 if B <= 8 else 4
    seqs = _mixed_seq(rs, B, T)
    bt = BatchedVitTracker(p, B)
    bt.initialize([s[0][0] for s in seqs], [s[1] for s in seqs])
    recs = np.stack([bt.track_record([s[0][t] for s in seqs]) for t in range(1, T)])
    check = range(B) if B <= 8 else [0, 1, 2, 3, 4, 5, 131, 255]
    for b in check:
        assert np.array_equal(recs[:, b], _solo(p, B, *seqs[b])), b


def test_slot_restart_equals_fresh_solo_trackers_and_leaves_the_others_alone():
    import torch
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.native import VtError
    p = _params("vit_48_h32_g128")
    B, T, R = 8, 8, 3             # restart after frame R
    rs = np.random.RandomState(6)
    seqs = _mixed_seq(rs, B, T)
    new = _mixed_seq(np.random.RandomState(7), B, T)
    slots = [0, 3, B - 1]

    def run(restart):
        bt = BatchedVitTracker(p, B)
        bt.initialize([s[0][0] for s in seqs], [s[1] for s in seqs])
        cur = [s[0] for s in seqs]
        recs = []
        for t in range(1, T):
            if restart and t == R:
                bt.reinitialize(slots, [new[b][0][0] for b in slots], [new[b][1] for b in slots])
                for b in slots:
                    cur[b] = [None] * (R - 1) + new[b][0]          # the new sequence's frame 1 at step R
            recs.append(bt.track_record([cur[b][t] for b in range(B)]))
        return np.stack(recs), bt

    base, _ = run(False)
    got, bt = run(True)
    for b in range(B):
        if b in slots:
            want = _solo(p, B, new[b][0][:T - R + 1], new[b][1])
            assert np.array_equal(got[R - 1:, b], want), b
            assert np.array_equal(got[:R - 1, b], base[:R - 1, b]), b
        else:
            assert np.array_equal(got[:, b], base[:, b]), b
    # vt_set_template_slots' argument and state checks
    z = torch.zeros(1, 3, p.template_size, p.template_size, device="cuda")
    for bad in ([B], [-1]):
        with pytest.raises(VtError, match=r"\(-1\)"):
            bt.nat.set_template_slots(z, bad)
    with pytest.raises(VtError, match=r"\(-1\)"):
        bt.nat.set_template_slots(torch.zeros(2, 3, p.template_size, p.template_size, device="cuda"), [1, 1])
    m = _model(128, 4)
    with pytest.raises(VtError, match=r"\(-3\)"):
        m.set_template_slots(z, [0])                     # no cache yet
    m.set_template(torch.zeros(4, 3, 64, 64, device="cuda"))
    m.set_form_batch(8)
    with pytest.raises(VtError, match=r"\(-3\)"):
        m.set_template_slots(z, [0])                     # the form batch changed since the cache was written


def _tracker(tmp_path, monkeypatch):
    from vittracker_amd.evaluation import Tracker
    monkeypatch.setenv("VITTRACK_SAVE_DIR", str(tmp_path))
    monkeypatch.setenv("VITTRACK_PRJ_DIR", REPO)
    t = Tracker("vit_dist", "vit_48_h32_g128", "synthetic")
    get = t.get_parameters

    def params():
        q = get()
        q.allow_synthetic_weights = True
        return q
    t.get_parameters = params
    return t


def test_continuous_runner_writes_the_files_of_the_sequential_runner(tmp_path, monkeypatch):
    from vittracker_amd.evaluation import get_dataset
    from vittracker_amd.evaluation.running import run_dataset, run_dataset_batched, run_dataset_continuous
    ds = get_dataset("synthetic_mixed:10x6")
    ts = _tracker(tmp_path / "seq", monkeypatch)
    run_dataset(ds, [ts], debug=False, threads=0)
    tc = _tracker(tmp_path / "cont", monkeypatch)
    run_dataset_continuous(ds, tc, batch=4)
    tb = _tracker(tmp_path / "grp", monkeypatch)
    run_dataset_batched(ds, tb, batch=4)
    for s in ds:
        a = open(os.path.join(ts.results_dir, s.name + ".txt")).read()
        assert len(a.splitlines()) == len(s), s.name
        assert open(os.path.join(tc.results_dir, s.name + ".txt")).read() == a, s.name
        assert open(os.path.join(tb.results_dir, s.name + ".txt")).read() == a, s.name
        tl = open(os.path.join(tc.results_dir, s.name + "_time.txt")).read().splitlines()
        assert len(tl) == len(s) and all(float(v) > 0 for v in tl)
