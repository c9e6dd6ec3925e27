"""GPU: tracking/test.py-style runs end to end on synthetic sequences (sequential plugin trackers vs the lock-step
batched runner: the result files must be identical), run_video through the real plugin, and the deployment session
against the reference-generated golden maps."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, REPO, load_case

pytestmark = pytest.mark.gpu


def _tracker(tmp_path, monkeypatch, yaml_name="vit_48_h32_g128"):
    from vittracker_amd.evaluation import Tracker
    monkeypatch.setenv("VITTRACK_SAVE_DIR", str(tmp_path))
    monkeypatch.setenv("VITTRACK_PRJ_DIR", REPO)
    t = Tracker("vit_dist", yaml_name, "synthetic")
    get = t.get_parameters

    def params():
        p = get()
        p.allow_synthetic_weights = True
        return p
    t.get_parameters = params
    return t


def test_sequential_and_batched_runs_write_identical_box_files(tmp_path, monkeypatch):
    from vittracker_amd.evaluation import get_dataset
    from vittracker_amd.evaluation.running import run_dataset, run_dataset_batched
    ds = get_dataset("synthetic:5x6")                       # ragged lengths 6, 8, 10, 6, 8
    ts = _tracker(tmp_path / "seq", monkeypatch)
    run_dataset(ds, [ts], debug=False, threads=0)
    tb = _tracker(tmp_path / "bat", monkeypatch)
    run_dataset_batched(ds, tb, batch=4)                    # groups of 4 + 1
    for s in ds:
        a = open(os.path.join(ts.results_dir, s.name + ".txt")).read()
        b = open(os.path.join(tb.results_dir, s.name + ".txt")).read()
        assert a == b and len(a.splitlines()) == len(s), s.name
        tl = open(os.path.join(tb.results_dir, s.name + "_time.txt")).read().splitlines()
        assert len(tl) == len(s) and all(float(v) > 0 for v in tl)
    tc = _tracker(tmp_path / "chunk", monkeypatch)
    run_dataset_batched(ds, tc, batch=4, frames_per_launch=3)     # 3 frames per graph launch: the same files again
    for s in ds:
        assert open(os.path.join(tc.results_dir, s.name + ".txt")).read() == open(os.path.join(tb.results_dir, s.name + ".txt")).read()
    for shards, n in ((2, 1), (3, 2)):                            # sub-groups on their own streams (ShardedBatchedTracker): the same files again
        tsd = _tracker(tmp_path / f"shards{shards}", monkeypatch)
        run_dataset_batched(ds, tsd, batch=4, frames_per_launch=n, shards=shards)
        for s in ds:
            assert open(os.path.join(tsd.results_dir, s.name + ".txt")).read() == open(os.path.join(tb.results_dir, s.name + ".txt")).read()
    # the target really is tracked on these textures? no: weights are synthetic -- only consistency is asserted


def test_run_video_through_the_plugin(tmp_path, monkeypatch):
    from vittracker_amd.evaluation.data import synthetic_sequence
    t = _tracker(tmp_path, monkeypatch, "vit_48_h32_noKD")
    seq = synthetic_sequence("clip", 6)
    np.save(tmp_path / "clip.npy", np.stack(seq.frames))
    box0 = seq.init_info()["init_bbox"]
    boxes = t.run_video(str(tmp_path / "clip.npy"), optional_box=box0, save_results=True)
    assert len(boxes) == 6 and all(isinstance(v, int) for v in boxes[1])
    rows = open(os.path.join(t.results_dir, "video_clip.txt")).read().splitlines()
    assert len(rows) == 6 and rows[1] == "\t".join(str(v) for v in boxes[1])
    # same boxes as the sequence loop (which also feeds RGB arrays here)
    out = t.run_sequence(seq)
    assert [[int(v) for v in b] for b in out["target_bbox"][1:]] == boxes[1:]


def test_deploy_session_matches_reference_golden_maps():
    from vittracker_amd import deploy
    g, sd, z, x = load_case(os.path.join(GOLDEN_DIR, "ref_G256_s1_b1.npz"))
    sess = deploy.VitTrackSession(sd)
    assert [i.name for i in sess.get_inputs()] == ["template", "search"]
    o1, o2, o3 = sess.run(None, {"template": z, "search": x})
    assert o1.shape == (1, 1, 16, 16) and o2.shape == (1, 2, 16, 16) and o3.shape == (1, 2, 16, 16)
    np.testing.assert_allclose(o1, g["score_map"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(o2, g["size_map"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(o3, g["offset_map"], atol=1e-4, rtol=0)
    (only3,) = sess.run(["output3"], {"template": z, "search": x})
    np.testing.assert_array_equal(only3, o3)
    with pytest.raises(ValueError, match="invalid dimensions"):
        sess.run(None, {"template": x, "search": x})
    with pytest.raises(ValueError, match="missing"):
        sess.run(None, {"template": z})
    with pytest.raises(ValueError, match="Invalid output name"):
        sess.run(["output4"], {"template": z, "search": x})


def test_bench_record_graph_form_on_one_gpu():
    """The launch form bench.py uses for N > 1 (graphs writing their result records straight into the all_gather buffers, S steps
    per launch + single-step remainder) run on one GPU without a communicator: records == plain forward (bench checks), rc 0."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--record-graphs", "--steps", "11", "--warmup", "3", "--batch", "32",
                        "--full", "--no-cpu", "--no-extra"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["checked"] and j["value"] > 0 and j["config"]["steps_per_graph"] == 4 and j["steps"] == 11


@pytest.mark.parametrize("streams", ["1", "2"])
def test_bench_plain_run_times_steps_and_dumps_the_last_outputs(tmp_path, streams):
    """A plain bench run (no --full) times exactly --steps steps in one region and, with --dump-outputs, writes the outputs of the
    last timed step: every shard's seeded inputs through the numpy oracle give the same maps and boxes."""
    import json
    import subprocess
    import sys
    from oracle import vt_oracle_np as onp
    from vittracker_amd import synth
    B, d = 8, tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", str(B),
                        "--streams", streams, "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == 7 and j["regions"]["n"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0 and not j["checked"]
    sd = synth.synth_state_dict(0, len_z=16, len_x=64)
    refs = [onp.forward(sd, *synth.synth_inputs(1000 * k, B, 64, 128)) for k in range(int(streams))]
    for k, tol in (("score_map", 1e-4), ("size_map", 1e-4), ("offset_map", 1e-4), ("pred_boxes", 1e-5), ("hann_boxes", 1e-5), ("conf", 1e-4)):
        got = np.load(d / (k + ".npy"))
        want = np.concatenate([ref[k].reshape((B,) + got.shape[1:]) for ref in refs])
        assert got.dtype == np.float32 and got.shape[0] == B * int(streams), (k, got.dtype, got.shape)
        assert float(np.abs(got - want).max()) < tol, k


@pytest.mark.parametrize("streams", ["1", "2"])
def test_bench_force_gather_runs_the_rccl_leg_on_one_gpu(streams):
    """Round 3 review: the RCCL leg of bench.py (init_process_group('nccl'), all_gather_into_tensor(async_op=True) per launch unit under
    the shard's stream, record graphs writing straight into the gather buffers) had only ever run on gloo.  --force-gather starts the
    single rank under torch.distributed.run (before any GPU call), builds a 1-rank RCCL communicator and runs exactly that form;
    bench.py itself checks gathered == the records the graphs wrote == a plain forward."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--force-gather", "--streams", streams, "--steps", "43",
                        "--warmup", "9", "--full", "--no-cpu", "--no-extra"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["checked"] and j["value"] > 0 and j["n_gpus"] == 1 and j["steps"] == 43
    assert j["gather"]["backend"] == "nccl" and j["gather"]["ranks"] == 1 and j["gather"]["records_checked"]
    assert "gather_exposed_us_per_step" in j and j["config"]["streams"] == int(streams)


def test_force_gather_form_is_as_fast_as_the_plain_form():
    """N = 1 with the real collective agrees with the plain form within 3 % (best of three alternating runs each)."""
    import json
    import subprocess
    import sys

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "400", "--warmup", "50", "--full", "--no-cpu", "--no-extra"] + extra,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"]
    plain, gat = [], []
    for _ in range(3):
        plain.append(run([]))
        gat.append(run(["--gpus", "1", "--force-gather"]))
    assert abs(max(gat) / max(plain) - 1.0) < 0.03, (plain, gat)


def test_record_graph_form_is_as_fast_as_the_plain_form():
    """SCALE N = 1 must agree with BENCH: at the metric's batch the record-graph launch form (what every rank runs when N > 1)
    and the plain form report the same frames/s (best of three alternating runs each, within 3 %)."""
    import json
    import subprocess
    import sys

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "400", "--warmup", "50", "--full", "--no-cpu", "--no-extra"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"]
    plain, rec = [], []
    for _ in range(3):
        plain.append(run([]))
        rec.append(run(["--record-graphs"]))
    assert abs(max(rec) / max(plain) - 1.0) < 0.03, (plain, rec)


@pytest.mark.parametrize("geom", ["G128", "G256"])
def test_two_shards_on_two_streams_equal_their_sequential_runs(geom):
    """bench.py's default launch pattern (--streams 2): two models -- two independent shards of sequences, each with its own
    workspaces and 4-step graph -- launched alternately on two HIP streams, so that kernels of both are resident on the chip at
    the same time.  Every output of every step must be bit-identical to the same model run alone."""
    import torch
    import bench
    B = 256 if geom == "G128" else 96
    rs = [bench.Runner(geom, B, seed=5 + 11 * k, steps_per_graph=4) for k in range(2)]
    want = []
    for r in rs:                                   # alone, eager
        out = r.model.forward(r.z, r.x)
        torch.cuda.synchronize()
        want.append({k: getattr(out, k).clone() for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")})
    for rep in range(30):                          # interleaved, several launches in flight on each stream
        for r in rs:
            r.graph_s.launch(r.stream)
    torch.cuda.synchronize()
    for r, w in zip(rs, want):
        for o in r.outs:                           # the four steps of the last graph launch
            for k, v in w.items():
                assert torch.equal(getattr(o, k), v), (geom, k)
    assert not torch.equal(want[0]["score_map"], want[1]["score_map"])
    for r in rs:
        r.close()


def test_sharded_batched_tracker_equals_one_batched_tracker():
    """ShardedBatchedTracker: B sequences as two / three groups on their own streams give, sequence by sequence and frame by frame,
    exactly what one BatchedVitTracker of B sequences gives (device frames, host frames, chunks)."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker, ShardedBatchedTracker
    from vittracker_amd.parameter import vit_dist as P
    os.environ.setdefault("VITTRACK_PRJ_DIR", REPO)
    p = P.parameters("vit_48_h32_g128")
    p.allow_synthetic_weights = True
    B, H, W = 10, 120, 160
    rs = np.random.RandomState(3)
    frames = rs.randint(0, 256, (7, B, H, W, 3)).astype(np.uint8)
    boxes = np.stack([rs.uniform(20, 90, B), rs.uniform(20, 60, B), rs.uniform(15, 40, B), rs.uniform(15, 40, B)], 1)
    one = BatchedVitTracker(p, B)
    one.initialize(frames[0], boxes)
    want = [one.track(frames[t])["target_bbox"].numpy().copy() for t in (1, 2)]
    want += list(one.track_chunk(frames[3:6])["target_bbox"].numpy().copy())
    want.append(one.track(torch.from_numpy(frames[6]).cuda())["target_bbox"].numpy().copy())
    for shards in (2, 3):
        sh = ShardedBatchedTracker(p, B, shards)
        assert sum(sh.sizes) == B and len(sh.trackers) == shards
        sh.initialize(frames[0], boxes)
        got = [sh.track(frames[t])["target_bbox"].numpy().copy() for t in (1, 2)]
        got += list(sh.track_chunk(frames[3:6])["target_bbox"].numpy().copy())
        got.append(sh.track(torch.from_numpy(frames[6]).cuda())["target_bbox"].numpy().copy())
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)



@pytest.mark.parametrize("yaml_name,B,shards", [("vit_48_h32_g128", 256, 4), ("vit_48_h32_noKD", 256, 2)])
def test_sharding_a_full_group_does_not_change_its_results(yaml_name, B, shards):
    """Round 3 advisor: the library picks a stage's kernel form by batch size (frame forms above 80 / 128 / 176 sequences, tile and
    multi-workgroup forms below), and two forms agree to fp32 rounding only -- so 256 sequences as two models of 128 ran other
    kernels than one model of 256.  Every shard now selects its forms by the WHOLE group's size (vt_set_form_batch): boxes and
    confidences of the sharded run equal the unsharded run bit for bit, at the full batch, at both geometries; and a shard that
    does NOT know the group's size (form_batch = 0) is shown to run different forms (else this test would prove nothing)."""
    import torch
    from vittracker_amd.batched import BatchedVitTracker, ShardedBatchedTracker
    from vittracker_amd.parameter import vit_dist as P
    os.environ.setdefault("VITTRACK_PRJ_DIR", REPO)
    p = P.parameters(yaml_name)
    p.allow_synthetic_weights = True
    H, W = 96, 128
    rs = np.random.RandomState(11)
    frames = rs.randint(0, 256, (4, B, H, W, 3)).astype(np.uint8)
    boxes = np.stack([rs.uniform(20, 70, B), rs.uniform(20, 50, B), rs.uniform(15, 40, B), rs.uniform(15, 40, B)], 1)

    def run(bt):
        bt.initialize(frames[0], boxes)
        out = []
        for t in (1, 2, 3):
            r = bt.track(frames[t])
            out.append((r["target_bbox"].numpy().copy(), r["confidence"].numpy().copy()))
        return out
    want = run(BatchedVitTracker(p, B))
    got = run(ShardedBatchedTracker(p, B, shards))      # shards of 64 (G128) / 128 (G256): batches that would pick the tile-form blocks
    for (wb, wc), (gb, gc) in zip(want, got):
        np.testing.assert_array_equal(wb, gb)
        np.testing.assert_array_equal(wc, gc)
    # the control: a shard-size tracker left to choose its forms by its own batch is NOT bit-identical to its part of the group
    n = B // shards
    part = BatchedVitTracker(p, n)
    part.initialize(frames[0][:n], boxes[:n])
    r = part.track(frames[1][:n])
    assert not np.array_equal(r["confidence"].numpy(), want[0][1][:n])
    np.testing.assert_allclose(r["confidence"].numpy(), want[0][1][:n], atol=1e-4)
