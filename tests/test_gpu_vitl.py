"""GPU: the ViT-Large OSTrack model point (width 1024, 16 heads of 64, depth 24, MLP 4096) at 128 / 256 and 192 / 384 -- the ViT-Base
kernels at a second width (vitb.hip: VbModel::C / HEADS / HID), bf16 MFMA against fp32 references.

References: tests/golden/ref_vitl_*.npz / ref_vl384_*.npz = outputs of the reference's own build_ostrack for vit_large_patch16_224
(tests/golden/make_golden_vitl.py) on the samples `rows` of a seed's 16-sample pool, every one with raw and Hann top-2 margins above
0.045 (the ViT-Base rule of 0.03 x sqrt(24 / 12)) -- the tests run exactly `rows` and excuse no argmax flip; the pinned torch oracle for
the activations that feed single stages.

Tolerances (tests/vitl_cases.py): the stated bf16 law of tests/test_gpu_vitb.py as written there, TOL_REL(n) = 2.0e-3 sqrt(n) on the
residual stream after n blocks against the rows' centred norm (its per-block term is relative: it does not depend on the width); 3.2e-3
on the token stage; 2e-4 on the f32 final norm; maps and boxes the ViT-Base bounds x sqrt(24 / 12), because the head reads features
that carry TOL_REL(24) instead of TOL_REL(12): score / size 3.1e-2, offset 6.2e-2, boxes 1.3e-2.
Measured on MI355X (this module's printed figures):
  residual stream after 1 / 6 / 12 / 24 blocks  1.18e-3 / 2.69e-3 / 3.52e-3 / 4.12e-3 at 256, 1.13e-3 / 2.61e-3 / 3.41e-3 / 4.28e-3 at 384
                                                (bounds 2.0e-3 / 4.9e-3 / 6.9e-3 / 9.8e-3); single blocks 12 / 23: 8.2e-4 / 6.6e-4 (384: 8.4e-4 / 6.8e-4)
  tokens 2.33e-3 (384: 2.34e-3); uint8 route 1.76e-3 / 1.62e-3
  maps over the four fixtures: score 1.80e-2, size 1.19e-2, offset 3.21e-2; boxes 6.0e-3 (pred), 8.4e-3 (Hann); uint8 fixture 1.35e-2 / 8.9e-3 /
  2.40e-2, boxes 2.5e-3

No tracking fixture exists: make_golden_vitl.py found no seed in its 40-seed range whose eight Hann margins all exceed 0.045
(tests/test_vitl_host.py pins that), so the tracking step is held by its exactness properties and the front-end test.
Exactness claims are torch.equal.  Depth-24 models are built once per (seed, geometry) for the whole module; everything that needs no
reference fixture runs a depth-2 model."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO
from vitb_u8_fold import MEAN, STD, TOL_TOKENS, rel_c
from vitl_cases import C, GEO, HEADS, TOL_BOX, TOL_MAP, TOL_REL, all_plain, load_plain, load_u8, plain_files, sd_vitl, u8_files

pytestmark = pytest.mark.gpu

KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
_MODELS = {}


def _new_model(geo, B, depth, sd):
    from vittracker_amd import native
    m = native.Model(GEO[geo]["TZ"], GEO[geo]["TX"], channels=C, heads=HEADS, depth=depth, head_channels=256, max_batch=B)
    m.load_state_dict(sd)
    return m


def _model(geo, B, seed, depth=24):
    """One model per (geometry, batch, weights, depth) for the whole module."""
    key = (geo, B, seed, depth)
    if key not in _MODELS:
        _MODELS[key] = _new_model(geo, B, depth, sd_vitl(seed, geo, depth))
    m = _MODELS[key]
    m.set_open_loop(False)
    return m


def _inputs(seed, B, geo="256"):
    import torch
    from vittracker_amd import synth
    z, x = synth.synth_inputs(seed, B, GEO[geo]["TZ"], GEO[geo]["TX"])
    return torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()


def _clone(o, keys=KEYS):
    from types import SimpleNamespace
    return SimpleNamespace(**{k: getattr(o, k).clone() for k in keys})


def _same(a, b, keys=KEYS):
    import torch
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def _against_fixture(out, g, tag, n=None):
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k][:n]).max())
        print(tag, k, err)
        assert err < tol, (k, err)
    eb = float(np.abs(out.pred_boxes.cpu().numpy() - g["pred_boxes"][:n, 0]).max())
    eh = float(np.abs(out.hann_boxes.cpu().numpy() - g["hann_boxes"][:n]).max())
    ec = float(np.abs(out.conf.cpu().numpy() - g["conf"][:n]).max())
    print(tag, "pred_boxes", eb, "hann_boxes", eh, "conf", ec)
    assert eb < TOL_BOX and eh < TOL_BOX and ec < TOL_MAP["score_map"], (eb, eh, ec)


# ------------------------------------------------------------------------------------------------- 1. fixture comparison
@pytest.mark.parametrize("geo,path", all_plain(), ids=lambda v: os.path.basename(v)[:-4] if v.endswith(".npz") else v)
def test_forward_matches_the_reference_fixture(geo, path):
    import torch
    g, sd, z, x = load_plain(geo, path)
    B, F = int(g["B"]), GEO[geo]["F"]
    m = _model(geo, B, int(g["seed"]))
    assert m.channels == C
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    out = m.forward(zd, xd)
    assert out.score_map.shape == (B, 1, F, F)
    _against_fixture(out, g, os.path.basename(path))
    bbox, mx = m.cal_bbox(out.score_map, out.size_map, out.offset_map)      # the boxes are the decode of THIS path's own maps
    assert torch.equal(bbox, out.pred_boxes) and torch.equal(mx, out.conf)
    graph, o2 = m.capture(zd, xd)                                            # graph replay == eager, bit for bit
    graph.launch()
    torch.cuda.synchronize()
    _same(out, o2)
    del graph


# ------------------------------------------------------------------------------------------------- 2. stages
_ACTS = {}


def _oracle_acts(geo):
    """The pinned oracle's full activations of the first sample of the geometry's activation fixture."""
    import torch
    from oracle import vitb_oracle_torch as ob
    if geo not in _ACTS:
        g, sd, z, x = load_plain(geo, plain_files(geo)[0])
        acts = {}
        with torch.no_grad():
            ob.build_from_state(sd, heads=HEADS)(torch.from_numpy(z[:1]), torch.from_numpy(x[:1]), acts)
        _ACTS[geo] = acts
    return _ACTS[geo]


def _one_block_model(geo, sd, k, B=1):
    """A depth-1 model carrying block k's weights."""
    return _new_model(geo, B, 1, {**sd, **{kk.replace(f"blocks.{k}.", "blocks.0."): v for kk, v in sd.items() if f"backbone.blocks.{k}." in kk}})


@pytest.mark.parametrize("geo", ["256", "384"])
def test_each_stage_against_reference_activations(geo):
    """Every stage fed the pinned oracle's upstream activation, its output held to the reference's stored rows: the patch embedding,
    blocks[0..k) for k = 1, 6, 12, 24, a single block at index 12 and one at 23, the final norm, the head."""
    import torch
    g, sd, z, x = load_plain(geo, plain_files(geo)[0])
    assert "act_norm" in g
    LZ, rows = GEO[geo]["LZ"], g["act_rows"]
    acts = _oracle_acts(geo)
    m = _model(geo, int(g["B"]), int(g["seed"]))
    tok = m.stem(torch.from_numpy(z[:1]).cuda(), torch.from_numpy(x[:1]).cuda())
    e = rel_c(tok[:1, rows].cpu().numpy(), g["act_tokens"])
    print(geo, "tokens", e)
    assert e < 3.2e-3
    for k in (1, 6, 12, 24):                     # blocks[0..k) from the oracle's tokens
        _, resid = m.blocks(acts["tokens"].cuda().contiguous(), nblocks=k, want_resid=True)
        e = rel_c(resid[:1, rows].cpu().numpy(), g[f"act_block{k - 1}"])
        print(geo, "blocks [0,", k, ")", e, "bound", TOL_REL(k))
        assert e < TOL_REL(k), k
    for k in (12, 23):                           # a single block from the oracle's input of that block
        m1 = _one_block_model(geo, sd, k)
        _, resid = m1.blocks(acts[f"block{k - 1}"].cuda().contiguous(), nblocks=1, want_resid=True)
        e = rel_c(resid[:1, rows].cpu().numpy(), g[f"act_block{k}"])
        print(geo, "block", k, e, "bound", TOL_REL(1))
        assert e < TOL_REL(1), k
        del m1
    feat = m.blocks(acts["block23"].cuda().contiguous(), nblocks=0)          # final norm only: f32 arithmetic
    srows = [r - LZ for r in rows if r >= LZ]
    np.testing.assert_allclose(feat[:1, srows].cpu().numpy(), g["act_norm"][:, [i for i, r in enumerate(rows) if r >= LZ]], atol=2e-4, rtol=0)
    out = m.head(acts["norm"][:, LZ:].cuda().contiguous())                    # head from the oracle's normalised tokens
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k][:1]).max())
        print(geo, "head", k, err)
        assert err < tol, (k, err)


# ------------------------------------------------------------------------------------------------- 3. the route at 256
def test_fused_route_at_256_agrees_with_the_unfused_one(monkeypatch):
    """ViT-Large at 128 / 256 runs the qkv projection inside the attention kernel (vbq::qkv_attn_wide_kernel<1024>), as ViT-Base does there.
    One block (block 0's weights, the oracle's tokens) on that route and on qk GEMM + v GEMM + vba::attn_kernel<320, 64> (VB_FUSED_QKV=0,
    read at model creation): both inside TOL_REL(1) of the reference's rows and within TOL_REL(1) of each other.  (Measured: 1.18e-3 each against the fixture
    and 0.0 between them -- the two routes walk k in the same 64-deep tiles, apply rstd and bias by the same fma and share vb_attn.h's
    attention arithmetic, so equal bits are no sign of a switch that was not read.)"""
    import torch
    g, sd, z, x = load_plain("256", plain_files("256")[0])
    rows, tokens = g["act_rows"], _oracle_acts("256")["tokens"].cuda().contiguous()
    fused = _one_block_model("256", sd, 0)
    monkeypatch.setenv("VB_FUSED_QKV", "0")
    unfused = _one_block_model("256", sd, 0)
    monkeypatch.delenv("VB_FUSED_QKV")
    res = {}
    for name, m in (("fused", fused), ("unfused", unfused)):
        _, resid = m.blocks(tokens, nblocks=1, want_resid=True)
        res[name] = resid.cpu().numpy().astype(np.float64)
        e = rel_c(res[name][:1, rows], g["act_block0"])
        print(name, "against the fixture", e, "bound", TOL_REL(1))
        assert e < TOL_REL(1), name
    between = rel_c(res["fused"][0], res["unfused"][0])
    print("fused against unfused, all 320 rows", between)
    assert between < TOL_REL(1)


# ------------------------------------------------------------------------------------------------- 4.-6. shapes (depth 2)
def test_batch_invariance_odd_batch_and_single_frame():
    """Frames 0 and 4 of a batch of 5 (M = 1600 rows: no multiple of the 256-row GEMM tile) in a max_batch = 8 model equal the same frames
    run alone (B = 1), bit for bit."""
    import torch
    m = _model("256", 8, 26, depth=2)
    zd, xd = _inputs(3, 5)
    full = _clone(m.forward(zd, xd))
    assert torch.isfinite(full.score_map).all() and torch.isfinite(full.offset_map).all()
    for i in (0, 4):
        one = m.forward(zd[i:i + 1].contiguous(), xd[i:i + 1].contiguous())
        assert torch.isfinite(one.score_map).all()
        for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes"):
            assert torch.equal(getattr(one, k)[0], getattr(full, k)[i]), (i, k)


# The GEMMs of a block run 256 x 256 tiles on a persistent grid of one workgroup per CU (vitb.hip launch_gemm / persistent_grid: 256 on
# MI355X).  The narrowest ones (proj, fc2: N = 1024 = 4 tile columns) have more tiles than workgroups from 65 tile rows up:
# 320 B > 64 x 256 -> B = 52 (16640 rows, 65 x 4 = 260 tiles); fc1 (16 columns) has 1040 there.
B_TILES = 52


def test_several_tiles_per_workgroup_equal_the_frames_four_at_a_time():
    import torch
    m = _model("256", B_TILES, 26, depth=2)
    zd, xd = _inputs(7, B_TILES)
    full = _clone(m.forward(zd, xd))
    assert torch.isfinite(full.score_map).all()
    for i0 in (0, 24, B_TILES - 4):
        part = m.forward(zd[i0:i0 + 4].contiguous(), xd[i0:i0 + 4].contiguous())
        for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes"):
            assert torch.equal(getattr(part, k), getattr(full, k)[i0:i0 + 4]), (i0, k)


def test_replays_of_a_captured_step_are_bit_identical():
    import torch
    m = _model("256", B_TILES, 26, depth=2)
    zd, xd = _inputs(9, B_TILES)
    graph, out = m.capture(zd, xd)
    graph.launch()
    torch.cuda.synchronize()
    ref = _clone(out)
    assert torch.isfinite(ref.score_map).all()
    for _ in range(8):
        graph.launch()
        torch.cuda.synchronize()
        _same(out, ref)
    del graph


# ------------------------------------------------------------------------------------------------- 7. uint8 and tracking
def test_forward_u8_matches_the_reference_fixture():
    import torch
    g, sd, z, patches = load_u8(u8_files()[0])
    B, LZ, L = int(g["B"]), 64, 320
    m = _model("256", B, int(g["seed"]))
    assert m.patch_u8_supported(1) and m.patch_u8_supported(B)
    zd, pd = torch.from_numpy(z).cuda(), torch.from_numpy(patches).cuda()
    out = m.forward_u8(zd, pd)
    _against_fixture(out, g, "u8")
    bbox, mx = m.cal_bbox(out.score_map, out.size_map, out.offset_map)
    assert torch.equal(bbox, out.pred_boxes) and torch.equal(mx, out.conf)
    tok = torch.zeros(B, L, C, device="cuda")
    m.stem_u8(pd, tok)
    rows = g["act_rows"]
    sel = [i for i, r in enumerate(rows) if r >= LZ]
    for b in (0, 1):
        e = rel_c(tok[b, rows[sel]].cpu().numpy(), g["act_tokens"][b, sel])
        print("tokens sample", b, e)
        assert e < TOL_TOKENS, (b, e)
    assert not tok[:, :LZ].any()          # template rows are not this call's to write


def test_template_cache_and_slots_are_exact():
    """set_template(z); forward*(None, .) == forward*(z, .) bit for bit; set_template_slots of slots {0, 2} in a batch of 3 leaves slot 1's
    output bit-identical and equals a full set_template with those rows replaced."""
    import torch
    from vittracker_amd import synth
    B = 3
    m = _model("256", 8, 26, depth=2)
    zd, xd = _inputs(3, B)
    pd = torch.from_numpy(synth.synth_patches(3, B, 256)).cuda()
    m.set_template(_inputs(4, B)[0])      # another template in the cache: a call with z must not read it
    u_off, f_off = _clone(m.forward_u8(zd, pd)), _clone(m.forward(zd, xd))
    m.set_template(zd)
    u_on, f_on = _clone(m.forward_u8(None, pd)), _clone(m.forward(None, xd))
    _same(u_on, u_off)
    _same(f_on, f_off)
    assert torch.isfinite(u_on.score_map).all() and not torch.equal(u_on.score_map, f_on.score_map)
    z2 = _inputs(5, 2)[0]
    m.set_template_slots(z2, [0, 2])
    got = _clone(m.forward_u8(None, pd))
    zmix = zd.clone()
    zmix[0], zmix[2] = z2[0], z2[1]
    m.set_template(zmix)
    _same(_clone(m.forward_u8(None, pd)), got)
    for k in KEYS:
        assert torch.equal(getattr(got, k)[1], getattr(u_off, k)[1]), k
    assert not torch.equal(got.score_map[0], u_off.score_map[0]) and not torch.equal(got.score_map[2], u_off.score_map[2])


H, W, TZ, TX, F = 120, 160, 128, 256, 16


def _steps(m, B, mode):
    """Two tracking steps on fixed frames from fixed boxes: vt_track_step, or its parts composed from the stage calls."""
    import torch
    from vittracker_amd import native
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([[30 + (b % 40), 20 + (b % 30), 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)
    states = torch.from_numpy(boxes).cuda()
    z, rf = m.crop(frames[0], states, 2.0, TZ, MEAN, STD)
    m.set_template(z)
    x, out, rec = torch.empty(B, 3, TX, TX, device="cuda"), native.Outputs(B, F, "cuda"), torch.zeros(B, 5, dtype=torch.float64, device="cuda")
    patch = torch.empty(B, TX, TX, 3, dtype=torch.uint8, device="cuda")
    recs = []
    for f in (1, 2):
        if mode == "step":
            m.track_step(frames[f], states, 4.0, MEAN, STD, x, rf, out, record=rec)
            patch = x.view(torch.uint8).flatten()[: B * TX * TX * 3].view(B, TX, TX, 3).clone()
        else:
            m.crop_u8(frames[f], states, 4.0, TX, out=patch, resize_factor=rf)
            m.forward_u8(None, patch, out=out)
            m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, TX, H, W, margin=10)
        torch.cuda.synchronize()
        recs.append([rec.clone(), states.clone(), rf.clone(), patch.clone()] + [getattr(out, k).clone() for k in KEYS])
    return recs


def test_track_step_is_crop_u8_forward_u8_and_the_tail():
    """vt_track_step == vt_crop_u8 + vt_forward_u8(z = None) + vt_update_state_record at B = 2, bit for bit: records, states, resize
    factors, the patch in the workspace, maps and boxes."""
    import torch
    m = _model("256", 8, 26, depth=2)
    res = {mode: _steps(m, 2, mode) for mode in ("step", "calls")}
    for a, b in zip(res["step"], res["calls"]):
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(ta, tb), i
    assert torch.isfinite(res["step"][-1][0]).all() and not torch.equal(res["step"][0][1], res["step"][1][1])
    assert torch.equal(res["step"][0][0][:, :4], res["step"][0][1])


def test_two_chain_step_equals_the_one_chain_step(monkeypatch):
    """B = 64 is the smallest batch whose step runs as two chains (VT_GRAPH_CHAINS is read at model creation): it equals the
    VT_GRAPH_CHAINS=1 step of a second model on the same weights, bit for bit."""
    import torch
    B = 64
    two = _model("256", B, 26, depth=2)
    monkeypatch.setenv("VT_GRAPH_CHAINS", "1")
    one = _new_model("256", B, 2, sd_vitl(26, "256", 2))
    monkeypatch.delenv("VT_GRAPH_CHAINS")
    a, b = _steps(two, B, "step"), _steps(one, B, "step")
    for sa, sb in zip(a, b):
        for i, (ta, tb) in enumerate(zip(sa, sb)):
            assert torch.equal(ta, tb), i
    assert torch.isfinite(a[-1][0]).all()


# ------------------------------------------------------------------------------------------------- 8. front ends
def _params():
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitl_256")
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    return p


def test_batched_tracker_and_plugin_on_vitl_256():
    """The ostrack plugin on vitl_256 with synthetic weights: initialize + 3 track calls; BatchedVitTracker at B = 2 on the same synthetic
    frames gives, for that sequence, exactly the plugin's boxes and confidences."""
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.model_vitb import OSTrack as Net
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    seqs = [synthetic_sequence(f"s{q}", 4, seed=1000 * 206 + q) for q in range(2)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]
    bt = BatchedVitTracker(_params(), 2)
    assert isinstance(bt.net, Net) and bt.net.depth == 24 and bt.net.geom["channels"] == C
    bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
    recs = [bt.track_record(np.stack([s.frames[t] for s in seqs])).copy() for t in range(1, 4)]
    assert np.isfinite(np.asarray(recs)).all()
    del bt
    plugin_mod._PIPELINES.clear()
    tr = OSTrack(_params(), "synthetic")
    tr.initialize(seqs[0].frames[0], {"init_bbox": box0[0]})
    for t in range(1, 4):
        got = tr.track(seqs[0].frames[t])
        assert isinstance(got["confidence"], float)
        assert got["target_bbox"] == recs[t - 1][0][:4].tolist(), t
        assert got["confidence"] == float(np.float32(recs[t - 1][0][4])), t
    plugin_mod._PIPELINES.clear()


# ------------------------------------------------------------------------------------------------- 9. rejection
def test_rejects_depth_25_and_names_a_missing_key():
    from vittracker_amd import native
    with pytest.raises(native.VtError) as e:
        native.Model(128, 256, channels=C, heads=HEADS, depth=25, head_channels=256)
    msg = str(e.value)
    assert "unsupported ViT-Large configuration" in msg and "CHANNELS=1024" in msg and "HEADS=16" in msg and "depth <= 24" in msg, msg
    sd = dict(sd_vitl(26, "256", 2))
    del sd["backbone.blocks.1.mlp.fc2.bias"]
    m = native.Model(128, 256, channels=C, heads=HEADS, depth=2, head_channels=256)
    with pytest.raises(native.VtError) as e:
        m.load_state_dict(sd)
    assert "backbone.blocks.1.mlp.fc2.bias" in str(e.value)
    # every other 1024-wide configuration stays on the shape-generic surface: it is created, and is no ViT model
    L = native.lib()
    h = ctypes.c_void_p()
    c = native.VtConfig(128, 256, 1024, 8, 25, 256, 16, 1)
    assert L.vt_create(ctypes.byref(c), ctypes.byref(h)) != 0 and b"ViT-Large" not in L.vt_last_error()      # depth 25 > 12: the generic path's own refusal
