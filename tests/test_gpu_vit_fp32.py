"""GPU: the fp32-equivalent mode of the patch-16 ViT path (vt_set_precision(VT_PRECISION_FP32)) -- three-piece bf16 operands,
six terms per product, fp32 activations, attention, GELU and head -- against the float64 truth of oracle/vitb_oracle_torch.py.

The bound (tests/vit_fp32_cases.py): a key passes when the device's max error against the truth is at most 8 x E_ref, E_ref = the
reference's own fp32 error against the same truth, and within 1e-4 (maps) / 1e-5 (boxes).  No margin selection: every sample's boxes count.

  1  whole model   every fixture of the four widths at both geometries and ViT-Base's common-mode fixtures through vt_forward; the bf16
                   mode of the same model on the same inputs must NOT meet 8 x E_ref on the maps
  2  stages        vt_stem, vt_blocks(1 and all), vt_head from the oracle's features, at the fixtures' activation rows under 8 x the
                   fixture's own error there; one depth-1 model per width on the "peaked", "common_mode" (320 tokens) and "last_keys"
                   (720 tokens: the partial last key chunk) regimes of tests/bf16_budget.py against run(.., "truth"), under 8 x the fp32
                   oracle's own error
  3  uint8 entry   vt_forward_u8 on the four uint8 fixtures against the truth of the normalised crop
  4  plumbing      eager == captured == second replay; B = 66 in two chains == one chain (VT_GRAPH_CHAINS=1 in a fresh child process);
                   template cache on == off; vt_set_template_slots; vt_track_step == its parts; BatchedVitTracker slots == solo plugin
                   trackers; tracking/test.py --precision fp32 with and without --batch 2; a batch whose expanded fc2 operand passes
                   4 GiB (its GEMMs run as row chunks) == its frames three at a time.  All bit for bit
  5  the switch    bf16 outputs before and after a visit to fp32 mode are the same bits; the refusals and their messages; vt_precision

Measured on MI355X (this module's printed figures): whole model and uint8 entry, per fixture and key: FACTORS_SEEN in
tests/vit_fp32_cases.py (largest 3.06 on a map, 5.00 on a box); stages 0.30-0.72 of the reference's own error on tokens and residual rows,
the head from the oracle's features 1.30-2.44 on maps and up to 5.36 on a box; regimes 0.39-1.17.  The ViT-Large cases take 10-15 s each:
a depth-24 state dict and its float64 truth on the CPU."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_budget as bb
import vit_fp32_cases as vc
from conftest import REPO
from vitb_u8_fold import MEAN, STD

pytestmark = pytest.mark.gpu

OUT_KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")


def _clone(o):
    return {k: getattr(o, k).clone() for k in OUT_KEYS}


def _same(a, b):
    import torch
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]), k


def _check(name, out, tag=""):
    err, ref, bnd = vc.errors(out, name), vc.e_ref(name), vc.bound(name)
    print(name, tag, {k: "%.2f" % (err[k] / ref[k]) for k in vc.KEYS}, {k: "%.2e" % err[k] for k in vc.KEYS})
    for k in vc.KEYS:
        assert err[k] <= bnd[k], (name, tag, k, err[k], ref[k], err[k] / ref[k])
    return err


# ------------------------------------------------------------------------------------------ 1  whole model
@pytest.mark.parametrize("name", sorted(vc.PLAIN))
def test_forward_holds_the_fp32_bound_and_the_bf16_mode_does_not(name):
    import torch
    g, sd, z, x = vc.load(name)
    m = vc.model(name, z.shape[0])
    assert m.precision == "fp32"
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    _check(name, m.forward(zd, xd))
    m.set_precision("bf16")
    err, ref = vc.errors(m.forward(zd, xd), name), vc.e_ref(name)
    assert all(err[k] > vc.FACTOR * ref[k] for k in vc.MAPS), (name, err, ref)
    m.close()


# ------------------------------------------------------------------------------------------------ 2  stages
@pytest.mark.parametrize("name", vc.STAGES)
def test_each_stage_against_the_float64_activations(name):
    import torch
    g, sd, z, x = vc.load(name)
    _, (C, heads), geo, depth, _ = vc.spec(name)
    LZ = vc.GEO[geo]["LZ"]
    rows = g["act_rows"]
    acts = vc.truth(name)["acts"]
    m = vc.model(name, z.shape[0])
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()

    def hold(tag, got, key, r=rows):
        want = acts[key][0, r]
        e_ref = np.abs(g["act_" + key][0].astype(np.float64) - want).max()
        e = np.abs(got.astype(np.float64) - want).max()
        print(name, tag, "ratio %.2f  device %.3e  reference %.3e" % (e / e_ref, e, e_ref))
        assert e_ref > 0 and e <= vc.FACTOR * e_ref, (name, tag, e, e_ref)

    tok = m.stem(zd, xd)
    hold("tokens", tok[0, rows].cpu().numpy(), "tokens")
    _, resid = m.blocks(tok, nblocks=1, want_resid=True)
    hold("block0", resid[0, rows].cpu().numpy(), "block0")
    feat, resid = m.blocks(tok, nblocks=-1, want_resid=True)
    hold("block%d" % (depth - 1), resid[0, rows].cpu().numpy(), "block%d" % (depth - 1))
    srows = rows[rows >= LZ]
    want = acts["norm"][0, srows]
    e_ref = np.abs(g["act_norm"][0][rows >= LZ].astype(np.float64) - want).max()
    e = np.abs(feat[0, srows - LZ].cpu().numpy().astype(np.float64) - want).max()
    print(name, "norm", "ratio %.2f" % (e / e_ref))
    assert len(srows) and e <= vc.FACTOR * e_ref, (name, e, e_ref)
    # the head alone, from the oracle's features (the float64 norm rounded to fp32)
    of = torch.from_numpy(np.ascontiguousarray(acts["norm"][:, LZ:].astype(np.float32))).cuda()
    _check(name, m.head(of), "head")
    m.close()


@pytest.mark.parametrize("C", (1024, 768, 384, 192))
@pytest.mark.parametrize("regime,L", (("peaked", 320), ("common_mode", 320), ("last_keys", 720)))
def test_one_block_on_the_regimes_where_bf16_is_worst(C, regime, L):
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    w = bb.WIDTHS[C]
    sd, X = bb.regime(regime, L, w=w, B=2)
    truth = bb.run(sd, X, nblocks=1, mode="truth", w=w)[0][0]
    with torch.no_grad():
        ref = ob.build_from_state(sd, heads=w.heads).backbone.blocks[0](torch.from_numpy(X)).numpy()
    e_ref = np.abs(ref.astype(np.float64) - truth).max()
    tz, tx = bb.SIZES[L]
    m = native.Model(tz, tx, channels=C, heads=w.heads, depth=1, head_channels=256, max_batch=2, family="vit")
    m.load_state_dict(sd)
    m.set_precision("fp32")
    _, resid = m.blocks(torch.from_numpy(X).cuda(), nblocks=1, want_resid=True)
    e = np.abs(resid.cpu().numpy().astype(np.float64) - truth).max()
    print(C, regime, L, "ratio %.2f  device %.3e  fp32 oracle %.3e" % (e / e_ref, e, e_ref))
    assert e_ref > 0 and e <= vc.FACTOR * e_ref, (e, e_ref)
    m.set_precision("bf16")
    _, r16 = m.blocks(torch.from_numpy(X).cuda(), nblocks=1, want_resid=True)
    assert np.abs(r16.cpu().numpy().astype(np.float64) - truth).max() > vc.FACTOR * e_ref
    m.close()


# ------------------------------------------------------------------------------------------- 3  uint8 entry
@pytest.mark.parametrize("name", sorted(vc.U8))
def test_forward_u8_holds_the_fp32_bound(name):
    import torch
    g, sd, z, patches = vc.load(name)
    m = vc.model(name, z.shape[0])
    _check(name, m.forward_u8(torch.from_numpy(z).cuda(), torch.from_numpy(patches).cuda()), "u8")
    m.close()


# --------------------------------------------------------------------------------------------- 4  plumbing
_SMALL = {}


def _small(B, geo="256", C=192, heads=3, depth=2, seed=31):
    """A depth-2 ViT-Tiny model in fp32 mode on synthetic weights, one per (B, geometry) for the module."""
    from vittracker_amd import native, synth
    key = (B, geo, C, depth, seed)
    if key not in _SMALL:
        g = vc.GEO[geo]
        sd = synth.synth_vitb_state_dict(seed, C=C, depth=depth, heads=heads, len_z=g["LZ"], len_x=g["LX"])
        m = native.Model(g["TZ"], g["TX"], channels=C, heads=heads, depth=depth, head_channels=256, max_batch=B, family="vit")
        m.load_state_dict(sd)
        m.set_precision("fp32")
        _SMALL[key] = (m, sd)
    _SMALL[key][0].set_open_loop(False)
    return _SMALL[key][0]


def _inputs(seed, B, geo="256"):
    import torch
    from vittracker_amd import synth
    z, x = synth.synth_inputs(seed, B, vc.GEO[geo]["TZ"], vc.GEO[geo]["TX"])
    return torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()


@pytest.mark.parametrize("geo", ("256", "384"))
def test_eager_equals_captured_equals_second_replay(geo):
    import torch
    B = 3
    m = _small(B, geo)
    zd, xd = _inputs(5, B, geo)
    eager = _clone(m.forward(zd, xd))
    graph, o2 = m.capture(zd, xd)
    with pytest.raises(Exception, match="before capturing"):      # VT_ERR_STATE while a captured graph is alive
        m.set_precision("bf16")
    assert m._L.vt_set_precision(m._h, 0) == -3
    for _ in range(2):
        graph.launch()
        torch.cuda.synchronize()
        _same(eager, _clone(o2))
    assert torch.isfinite(eager["score_map"]).all()
    del graph
    _SMALL.pop((B, geo, 192, 2, 31))[0].close()


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_vit_fp32 as T
res = T._chains_run()
np.savez(sys.argv[1], **{k: v.cpu().numpy() for k, v in res.items()})
print("CHILD-OK")
"""


def _chains_run():
    """B = 66 through forward_u8 on the cached template: two chains from 64 frames up unless VT_GRAPH_CHAINS=1."""
    import torch
    from vittracker_amd import synth
    B = 66
    m = _small(B)
    m.set_template(torch.from_numpy(synth.synth_inputs(11, B, 128, 256)[0]).cuda())
    res = _clone(m.forward_u8(None, torch.from_numpy(synth.synth_patches(11, B, 256)).cuda()))
    _SMALL.pop((B, "256", 192, 2, 31))[0].close()
    return res


def test_two_chains_equal_one_chain(tmp_path):
    two = _chains_run()
    path = str(tmp_path / "one_chain.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % (REPO, os.path.join(REPO, "tests")), path], env=dict(os.environ, VT_GRAPH_CHAINS="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    one = np.load(path)
    for k, t in two.items():
        assert np.array_equal(one[k], t.cpu().numpy()), k
    assert np.isfinite(one["score_map"]).all()


def test_a_batch_whose_expanded_operand_passes_4_gib_equals_its_frames():
    """ViT-Large at 192 / 384, 124 frames, one block: fc2's expanded operand is 124 x 720 x 4096 x 12 = 4.39e9 bytes, more than the 32-bit byte
    offsets of one GEMM launch reach, so fc2 runs as two launches whose boundary (row 87296) lies inside frame 121.  Frames 0-2 and 121-123
    equal the same frames through a model of three, bit for bit."""
    import torch
    from vittracker_amd import native, synth
    B = 124
    sd = synth.synth_vitb_state_dict(41, C=1024, depth=1, heads=16, len_z=144, len_x=576)
    z, x = synth.synth_inputs(41, 8, 192, 384)
    idx = torch.arange(B) % 8
    zd, xd = torch.from_numpy(z).cuda()[idx].contiguous(), torch.from_numpy(x).cuda()[idx].contiguous()
    big = native.Model(192, 384, channels=1024, heads=16, depth=1, head_channels=256, max_batch=B)
    big.load_state_dict(sd)
    big.set_precision("fp32")
    out = _clone(big.forward(zd, xd))
    big.close()
    small = native.Model(192, 384, channels=1024, heads=16, depth=1, head_channels=256, max_batch=3)
    small.load_state_dict(sd)
    small.set_precision("fp32")
    for f0 in (0, 121):
        part = _clone(small.forward(zd[f0:f0 + 3].contiguous(), xd[f0:f0 + 3].contiguous()))
        for k in OUT_KEYS:
            assert torch.equal(out[k][f0:f0 + 3], part[k]), (f0, k)
    assert torch.isfinite(out["score_map"]).all()
    small.close()


def test_template_cache_and_slots_are_exact():
    import torch
    from vittracker_amd import synth
    B = 3
    m = _small(B)
    zd, xd = _inputs(3, B)
    pd = torch.from_numpy(synth.synth_patches(3, B, 256)).cuda()
    m.set_template(_inputs(4, B)[0])      # another template in the cache: a call with z must not read it
    u_off, f_off = _clone(m.forward_u8(zd, pd)), _clone(m.forward(zd, xd))
    m.set_template(zd)
    u_on, f_on = _clone(m.forward_u8(None, pd)), _clone(m.forward(None, xd))
    _same(u_on, u_off)
    _same(f_on, f_off)
    assert torch.isfinite(u_on["score_map"]).all() and not torch.equal(u_on["score_map"], f_on["score_map"])
    z2 = _inputs(5, 2)[0]
    m.set_template_slots(z2, [0, 2])
    got = _clone(m.forward_u8(None, pd))
    zmix = zd.clone()
    zmix[0], zmix[2] = z2[0], z2[1]
    _same(_clone(m.forward_u8(zmix, pd)), got)
    for k in OUT_KEYS:
        assert torch.equal(got[k][1], u_off[k][1]), k
    assert not torch.equal(got["score_map"][0], u_off["score_map"][0]) and not torch.equal(got["score_map"][2], u_off["score_map"][2])
    # the switch drops the cache: a cached call needs vt_set_template again
    m.set_precision("bf16")
    with pytest.raises(Exception, match="set_template"):
        m.forward(None, xd)
    m.set_precision("fp32")


H, W = 120, 160


def _steps(m, B, mode):
    import torch
    from vittracker_amd import native
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([[30 + (b % 40), 20 + (b % 30), 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)
    states = torch.from_numpy(boxes).cuda()
    z, rf = m.crop(frames[0], states, 2.0, 128, MEAN, STD)
    m.set_template(z)
    x, out = torch.empty(B, 3, 256, 256, device="cuda"), native.Outputs(B, 16, "cuda")
    rec, patch = torch.zeros(B, 5, dtype=torch.float64, device="cuda"), torch.empty(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
    recs = []
    for f in (1, 2):
        if mode == "step":
            m.track_step(frames[f], states, 4.0, MEAN, STD, x, rf, out, record=rec)
        else:
            m.crop_u8(frames[f], states, 4.0, 256, out=patch, resize_factor=rf)
            m.forward_u8(None, patch, out=out)
            m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, 256, H, W, margin=10)
        torch.cuda.synchronize()
        recs.append([rec.clone(), states.clone(), rf.clone()] + [getattr(out, k).clone() for k in OUT_KEYS])
    return recs


def test_track_step_is_crop_u8_forward_u8_and_the_tail():
    import torch
    B = 3
    m = _small(B)
    res = {mode: _steps(m, B, mode) for mode in ("step", "calls")}
    for a, b in zip(res["step"], res["calls"]):
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(ta, tb), i
    assert torch.isfinite(res["step"][-1][0]).all() and not torch.equal(res["step"][0][1], res["step"][1][1])


def _params(precision):
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitt_256")
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    p.precision = precision
    return p


def test_batched_tracker_slots_equal_solo_plugin_trackers(monkeypatch):
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    monkeypatch.delenv("VB_PRECISION", raising=False)
    seqs = [synthetic_sequence(f"s{q}", 4, seed=7000 + q) for q in range(2)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]
    recs = {}
    for prec in ("fp32", "bf16"):
        bt = BatchedVitTracker(_params(prec), 2)
        assert bt.net.precision == prec and bt.nat.precision == prec
        bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
        recs[prec] = [bt.track_record(np.stack([s.frames[t] for s in seqs])).copy() for t in range(1, 4)]
    assert not np.array_equal(recs["fp32"][0], recs["bf16"][0])
    plugin_mod._PIPELINES.clear()
    for q in range(2):
        tr = OSTrack(_params("fp32"), "synthetic")
        assert tr.network.precision == "fp32" and tr.network._native().precision == "fp32"
        tr.initialize(seqs[q].frames[0], {"init_bbox": box0[q]})
        for t in range(1, 4):
            got = tr.track(seqs[q].frames[t])
            assert got["target_bbox"] == recs["fp32"][t - 1][q][:4].tolist(), (q, t)
    plugin_mod._PIPELINES.clear()


@pytest.mark.parametrize("batch", ([], ["--batch", "2"]))
def test_the_evaluation_cli_runs_in_fp32_mode(tmp_path, batch):
    env = dict(os.environ, VITTRACK_SAVE_DIR=str(tmp_path), VITTRACK_PRJ_DIR=REPO)
    p = subprocess.run([sys.executable, os.path.join(REPO, "tracking", "test.py"), "ostrack", "vitb_256", "--dataset_name", "synthetic:2x4",
                        "--synthetic_weights", "--precision", "fp32"] + batch, env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    boxes = sorted(f for f in glob.glob(os.path.join(str(tmp_path), "**", "*.txt"), recursive=True)
                   if not f.endswith(("_time.txt", "_all_boxes.txt", "_all_scores.txt")))
    assert len(boxes) == 2, (boxes, p.stdout[-2000:] + p.stderr[-2000:])
    from vittracker_amd.evaluation.data import get_dataset
    frames = {s.name: len(s.frames) for s in get_dataset("synthetic:2x4")}
    assert sorted(os.path.basename(f)[:-4] for f in boxes) == sorted(frames)
    for f in boxes:          # the harness prints and skips a sequence that raises: one finite row per frame says it ran
        rows = [ln for ln in open(f).read().splitlines() if ln.strip()]
        assert len(rows) == frames[os.path.basename(f)[:-4]], (f, rows)
        assert np.isfinite(np.array([[float(v) for v in ln.replace(",", " ").split()] for ln in rows])).all()


# ------------------------------------------------------------------------------------------- 5  the switch
def test_bf16_results_are_the_same_bits_before_and_after_fp32_mode():
    import torch
    from vittracker_amd import native, synth
    B = 2
    sd = synth.synth_vitb_state_dict(26, depth=2)
    m = native.Model(128, 256, channels=768, heads=12, depth=2, head_channels=256, max_batch=B)
    assert m.precision == "bf16" and m._L.vt_precision(m._h) == 0
    m.set_precision("fp32")      # before vt_load_weights: the piece images are built by the load
    m.load_state_dict(sd)
    zd, xd = _inputs(26, B)
    f_first = _clone(m.forward(zd, xd))
    m.set_precision("bf16")
    before = _clone(m.forward(zd, xd))
    m.set_precision("fp32")
    assert m.precision == "fp32" and m._L.vt_precision(m._h) == 1
    f_second = _clone(m.forward(zd, xd))
    _same(f_first, f_second)
    m.set_precision("bf16")
    _same(before, _clone(m.forward(zd, xd)))
    assert not torch.equal(before["score_map"], f_second["score_map"])
    # a model that loads first and switches afterwards computes the same bits
    m2 = native.Model(128, 256, channels=768, heads=12, depth=2, head_channels=256, max_batch=B)
    m2.load_state_dict(sd)
    m2.set_precision("fp32")
    _same(f_first, _clone(m2.forward(zd, xd)))
    with pytest.raises(native.VtError, match="ViT precision"):
        m2.set_precision("f32")
    assert m2._L.vt_set_precision(m2._h, 7) == -1 and b"VT_PRECISION_FP32" in m2._L.vt_last_error()
    m.close()
    m2.close()


def test_refusals_and_their_messages(monkeypatch):
    from vittracker_amd import native, synth
    L = native.lib()
    v48 = native.Model(64, 128, max_batch=1)
    assert L.vt_set_precision(v48._h, 1) == -1 and b"patch-16 ViT" in L.vt_last_error()
    assert L.vt_precision(v48._h) == -1 and v48.precision == "f32"
    gen = native.Model(128, 256, channels=384, heads=6, depth=1, head_channels=256)      # vt_create at 384 / 6: a shape-generic vit_dist model
    assert L.vt_set_precision(gen._h, 1) == -1 and b"patch-16 ViT" in L.vt_last_error()
    m = native.Model(128, 256, channels=768, heads=12, depth=4, head_channels=256, max_batch=1)
    m.set_candidate_elimination([1], [0.7])
    assert L.vt_set_precision(m._h, 1) == -3 and b"candidate elimination" in L.vt_last_error() and b"fp32" in L.vt_last_error()
    assert m.precision == "bf16"
    m2 = native.Model(128, 256, channels=768, heads=12, depth=4, head_channels=256, max_batch=1)
    m2.set_precision("fp32")
    with pytest.raises(native.VtError, match="(?s)candidate elimination.*fp32"):
        m2.set_candidate_elimination([1], [0.7])
    assert m2.precision == "fp32"
    # VB_PRECISION is read at vt_create
    monkeypatch.setenv("VB_PRECISION", "fp32")
    m3 = native.Model(128, 256, channels=192, heads=3, depth=1, head_channels=256, max_batch=1, family="vit")
    monkeypatch.delenv("VB_PRECISION")
    assert m3.precision == "fp32"
    for x in (v48, gen, m, m2, m3):
        x.close()
