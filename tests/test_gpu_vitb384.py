"""GPU: the ViT-Base OSTrack path at the 384 geometry (192 px template / 384 px search: 144 + 576 = 720 tokens, 24 x 24 maps) and its
key-streaming attention kernel (vb_attn_stream.h), bf16 MFMA against fp32 references.

References: tests/golden/ref_vb384_*.npz = outputs of the reference's own build_ostrack at 192 / 384 (tests/golden/make_golden_vitb384.py)
on the samples `rows` of a seed's 16-sample batch, every one with raw and Hann top-2 margins above 0.03 -- the tests run exactly `rows`,
no sample is left out and no argmax flip is excused; the pinned torch oracle for the activations that feed single stages.

Tolerances are the ones tests/test_gpu_vitb.py states and derives: TOL_REL(n) = 2.0e-3 sqrt(n) on the residual stream after n blocks
(from the bf16 rounding model: it does not depend on the token count), 3.2e-3 on the token stage, 2e-4 on the f32 final norm, TOL_MAP /
TOL_BOX on maps and boxes.  A pad key (720 = 22 x 32 + 16: the last 32-key chunk is half empty) leaking into a softmax would move a
block's output by about 2 % and cannot pass TOL_REL.  Exactness claims are torch.equal.  Models of depth 12 are built once per module;
everything that is not a fixture comparison runs depth 2."""
import os

import numpy as np
import pytest

from conftest import REPO, load_vitb_case, vitb_golden_files
from test_gpu_vitb import TOL_BOX, TOL_MAP, TOL_REL
from test_vitb384_host import F, LX, LZ, TX, TZ, load_vb384, load_vb384_u8, sd384, vb384_files, vb384_u8_files
from vitb_u8_fold import MEAN, STD, TOL_TOKENS, rel_c

pytestmark = pytest.mark.gpu

KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
L = LZ + LX
_MODELS = {}


def _model(B, seed, depth=12):
    """One model per (batch, weights, depth) for the whole module."""
    from vittracker_amd import native
    key = (B, seed, depth)
    if key not in _MODELS:
        m = native.Model(TZ, TX, channels=768, heads=12, depth=depth, head_channels=256, max_batch=B)
        m.load_state_dict(sd384(seed, depth))
        _MODELS[key] = m
    m = _MODELS[key]
    m.set_open_loop(False)
    return m


def _inputs(seed, B):
    import torch
    from vittracker_amd import synth
    z, x = synth.synth_inputs(seed, B, TZ, TX)
    return torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()


def _clone(o, keys=KEYS):
    from types import SimpleNamespace
    return SimpleNamespace(**{k: getattr(o, k).clone() for k in keys})


def _same(a, b, keys=KEYS):
    import torch
    for k in keys:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def _against_fixture(out, g, tag):
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k]).max())
        print(tag, k, err)
        assert err < tol, (k, err)
    eb = float(np.abs(out.pred_boxes.cpu().numpy() - g["pred_boxes"][:, 0]).max())
    eh = float(np.abs(out.hann_boxes.cpu().numpy() - g["hann_boxes"]).max())
    ec = float(np.abs(out.conf.cpu().numpy() - g["conf"]).max())
    print(tag, "pred_boxes", eb, "hann_boxes", eh, "conf", ec)
    assert eb < TOL_BOX and eh < TOL_BOX and ec < TOL_MAP["score_map"], (eb, eh, ec)


# ------------------------------------------------------------------------------------------------- fixture comparison
@pytest.mark.parametrize("path", vb384_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_forward_matches_the_reference_fixture(path):
    import torch
    g, sd, z, x = load_vb384(path)
    m = _model(int(g["B"]), int(g["seed"]))
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    out = m.forward(zd, xd)
    assert out.score_map.shape == (int(g["B"]), 1, F, F)
    _against_fixture(out, g, os.path.basename(path))
    bbox, mx = m.cal_bbox(out.score_map, out.size_map, out.offset_map)      # the boxes are the decode of THIS path's own maps
    assert torch.equal(bbox, out.pred_boxes) and torch.equal(mx, out.conf)
    graph, o2 = m.capture(zd, xd)                                            # graph replay == eager, bit for bit
    graph.launch()
    torch.cuda.synchronize()
    _same(out, o2)


def test_each_stage_against_reference_activations():
    """As test_gpu_vitb.test_vitb_each_stage_against_reference_activations: every stage fed the pinned oracle's upstream activation, its
    output held to the reference's stored rows -- 0, 143 | 144, 145 (template / search boundary), 703 | 704 (both sides of the last whole
    32-key chunk), 719 and seven more."""
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    g, sd, z, x = load_vb384(vb384_files()[0])
    assert "act_norm" in g
    rows = g["act_rows"]
    z1, x1 = torch.from_numpy(z[:1]), torch.from_numpy(x[:1])
    acts = {}
    with torch.no_grad():
        ob.build_from_state(sd)(z1, x1, acts)
    m = _model(int(g["B"]), int(g["seed"]))
    tok = m.stem(z1.cuda(), x1.cuda())
    e = rel_c(tok[:1, rows].cpu().numpy(), g["act_tokens"])
    print("tokens", e)
    assert e < 3.2e-3
    for k in (1, 4, 12):                         # blocks[0..k) from the oracle's tokens
        _, resid = m.blocks(acts["tokens"].cuda().contiguous(), nblocks=k, want_resid=True)
        e = rel_c(resid[:1, rows].cpu().numpy(), g[f"act_block{k - 1}"])
        print("blocks [0,", k, ")", e, "bound", TOL_REL(k))
        assert e < TOL_REL(k), k
    for k in (5, 11):                            # a single block from the oracle's input of that block: a depth-1 model carrying block k's weights
        m1 = native.Model(TZ, TX, channels=768, heads=12, depth=1, head_channels=256, max_batch=1)
        m1.load_state_dict({**sd, **{kk.replace(f"blocks.{k}.", "blocks.0."): v for kk, v in sd.items() if f"backbone.blocks.{k}." in kk}})
        _, resid = m1.blocks(acts[f"block{k - 1}"].cuda().contiguous(), nblocks=1, want_resid=True)
        e = rel_c(resid[:1, rows].cpu().numpy(), g[f"act_block{k}"])
        print("block", k, e, "bound", TOL_REL(1))
        assert e < TOL_REL(1), k
    feat = m.blocks(acts["block11"].cuda().contiguous(), nblocks=0)          # final norm only: f32 arithmetic
    srows = [r - LZ for r in rows if r >= LZ]
    np.testing.assert_allclose(feat[:1, srows].cpu().numpy(), g["act_norm"][:, [i for i, r in enumerate(rows) if r >= LZ]], atol=2e-4, rtol=0)
    out = m.head(acts["norm"][:, LZ:].cuda().contiguous())                    # head from the oracle's normalised tokens
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k][:1]).max())
        print("head", k, err)
        assert err < tol, (k, err)


@pytest.mark.parametrize("path", vitb_golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_streaming_kernel_at_320_tokens_holds_the_256_fixtures(path, monkeypatch):
    """VB_FUSED_QKV=0 VB_ATTN_STREAM=1 (read at model creation): the 256 geometry on qk GEMM + v GEMM + vbs::attn_stream_kernel<320> -- five
    whole 64-key chunks, no partial one -- against the four ref_vitb_* fixtures at their own tolerances; one block against the stored
    activations at TOL_REL(1) where the fixture has them.  That the switch was honoured: a second model under VB_FUSED_QKV=0 alone
    (vba::attn_kernel<320, 64> on the same qk / vt) holds the same tolerances and does NOT give the same bits -- the two kernels round P
    against different maxima and accumulate in different orders."""
    import torch
    from oracle import vitb_oracle_torch as ob
    from vittracker_amd import native
    monkeypatch.setenv("VB_FUSED_QKV", "0")
    monkeypatch.setenv("VB_ATTN_STREAM", "1")
    g, sd, z, x = load_vitb_case(path)
    m = native.Model(128, 256, channels=768, heads=12, depth=12, head_channels=256, max_batch=int(g["B"]))
    m.load_state_dict(sd)
    out = m.forward(torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda())
    _against_fixture(out, g, "stream@320 " + os.path.basename(path))
    monkeypatch.delenv("VB_ATTN_STREAM")
    plain = native.Model(128, 256, channels=768, heads=12, depth=12, head_channels=256, max_batch=int(g["B"]))
    plain.load_state_dict(sd)
    pout = plain.forward(torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda())
    _against_fixture(pout, g, "unfused@320 " + os.path.basename(path))
    assert not torch.equal(pout.score_map, out.score_map) and not torch.equal(pout.offset_map, out.offset_map)
    monkeypatch.setenv("VB_ATTN_STREAM", "1")
    if "act_block0" in g:
        acts = {}
        with torch.no_grad():
            ob.build_from_state(sd)(torch.from_numpy(z[:1]), torch.from_numpy(x[:1]), acts)
        _, resid = m.blocks(acts["tokens"].cuda().contiguous(), nblocks=1, want_resid=True)
        e = rel_c(resid[:1, g["act_rows"]].cpu().numpy(), g["act_block0"])
        print("stream@320 one block", e)
        assert e < TOL_REL(1)


# ------------------------------------------------------------------------------------------------- shapes (depth 2)
def test_batch_invariance_odd_batch_and_single_frame():
    """Frames 0 and 4 of a batch of 5 (M = 3600 rows: no multiple of the 256-row GEMM tile) in a max_batch = 8 model equal the same frames
    run alone (B = 1), bit for bit."""
    import torch
    m = _model(8, 26, depth=2)
    zd, xd = _inputs(3, 5)
    full = _clone(m.forward(zd, xd))
    assert torch.isfinite(full.score_map).all() and torch.isfinite(full.offset_map).all()
    for i in (0, 4):
        one = m.forward(zd[i:i + 1].contiguous(), xd[i:i + 1].contiguous())
        assert torch.isfinite(one.score_map).all()
        for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes"):
            assert torch.equal(getattr(one, k)[0], getattr(full, k)[i]), (i, k)


def test_large_batch_equals_its_frames_four_at_a_time():
    """B = 24: 24 x 12 x 4 = 1152 attention workgroups (288 (frame, head) pairs, more than the chip's CUs) and several tiles per workgroup in
    every GEMM.  Frames 0-3 and 20-23 equal those frames run four at a time, bit for bit."""
    import torch
    B = 24
    m = _model(B, 26, depth=2)
    zd, xd = _inputs(7, B)
    full = _clone(m.forward(zd, xd))
    assert torch.isfinite(full.score_map).all()
    for i0 in (0, 20):
        part = m.forward(zd[i0:i0 + 4].contiguous(), xd[i0:i0 + 4].contiguous())
        for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes"):
            assert torch.equal(getattr(part, k), getattr(full, k)[i0:i0 + 4]), (i0, k)


@pytest.mark.parametrize("B,replays", [(5, 40), (24, 12)])
def test_replays_are_bit_identical_under_load(B, replays):
    """Race screen of the streaming kernel's double-buffered LDS-DMA (one barrier per chunk) and of the GEMMs at these shapes: replays of a
    captured step, a second stream multiplying a 256 MB buffer four times per replay meanwhile; EVERY replay's outputs are compared with
    the first one's, bit for bit, before the next replay overwrites them."""
    import torch
    m = _model(max(B, 8), 26, depth=2)
    zd, xd = _inputs(B + 3, B)
    graph, out = m.capture(zd, xd)
    graph.launch()
    torch.cuda.synchronize()
    ref = _clone(out)
    noise = torch.empty(64 << 20, device="cuda")
    side = torch.cuda.Stream()
    for it in range(replays):
        with torch.cuda.stream(side):
            for _ in range(4):
                noise.mul_(1.0001)
        graph.launch()
        torch.cuda.synchronize()
        _same(out, ref)
    del graph


# ------------------------------------------------------------------------------------------------- tracker
def test_forward_u8_matches_the_reference_fixture():
    import torch
    g, sd, z, patches = load_vb384_u8(vb384_u8_files()[0])
    B = int(g["B"])
    m = _model(B, int(g["seed"]))
    assert m.patch_u8_supported(1) and m.patch_u8_supported(B)
    zd, pd = torch.from_numpy(z).cuda(), torch.from_numpy(patches).cuda()
    out = m.forward_u8(zd, pd)
    _against_fixture(out, g, "u8")
    bbox, mx = m.cal_bbox(out.score_map, out.size_map, out.offset_map)
    assert torch.equal(bbox, out.pred_boxes) and torch.equal(mx, out.conf)
    tok = torch.zeros(B, L, 768, device="cuda")
    m.stem_u8(pd, tok)
    rows = g["act_rows"]
    sel = [i for i, r in enumerate(rows) if r >= LZ]
    for b in (0, 1):
        e = rel_c(tok[b, rows[sel]].cpu().numpy(), g["act_tokens"][b, sel])
        print("tokens sample", b, e)
        assert e < TOL_TOKENS, (b, e)
    assert not tok[:, :LZ].any()          # template rows are not this call's to write


def test_template_cache_and_slots_are_exact():
    """set_template(z); forward*(None, .) == forward*(z, .) bit for bit (the cache is max_batch x 144 operand rows); set_template_slots of slots
    {0, 2} in a batch of 3 leaves slot 1's output bit-identical and equals a full set_template with those rows replaced."""
    import torch
    from vittracker_amd import synth
    B = 3
    m = _model(8, 26, depth=2)
    zd, xd = _inputs(3, B)
    pd = torch.from_numpy(synth.synth_patches(3, B, TX)).cuda()
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
    _same(_clone(m.forward_u8(zmix, pd)), got)
    for k in KEYS:
        assert torch.equal(getattr(got, k)[1], getattr(u_off, k)[1]), k
    assert not torch.equal(got.score_map[0], u_off.score_map[0]) and not torch.equal(got.score_map[2], u_off.score_map[2])


H, W = 120, 160


def _frames_boxes(B, n, seed=8):
    import torch
    rs = np.random.RandomState(seed)
    frames = torch.from_numpy(rs.randint(0, 256, (n, B, H, W, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([[30 + (b % 40), 20 + (b % 30), 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)
    return frames, boxes


def _start(m, frames, boxes):
    import torch
    from vittracker_amd import native
    B = boxes.shape[0]
    states = torch.from_numpy(boxes).cuda()
    z, rf = m.crop(frames[0], states, 2.0, TZ, MEAN, STD)
    assert z.shape == (B, 3, TZ, TZ)
    m.set_template(z)
    return (states, rf, torch.empty(B, 3, TX, TX, device="cuda"), native.Outputs(B, F, "cuda"), torch.zeros(B, 5, dtype=torch.float64, device="cuda"))


def _steps(m, B, mode):
    """Two tracking steps on fixed frames from fixed boxes: vt_track_step, or its parts composed from the stage calls."""
    import torch
    frames, boxes = _frames_boxes(B, 3)
    states, rf, x, out, rec = _start(m, frames, boxes)
    patch = torch.empty(B, TX, TX, 3, dtype=torch.uint8, device="cuda")
    recs = []
    for f in (1, 2):
        if mode == "step":
            m.track_step(frames[f], states, 5.0, MEAN, STD, x, rf, out, record=rec)
            patch = x.view(torch.uint8).flatten()[: B * TX * TX * 3].view(B, TX, TX, 3).clone()
        else:
            m.crop_u8(frames[f], states, 5.0, TX, out=patch, resize_factor=rf)
            m.forward_u8(None, patch, out=out)
            m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, TX, H, W, margin=10)
        torch.cuda.synchronize()
        recs.append([rec.clone(), states.clone(), rf.clone(), patch.clone()] + [getattr(out, k).clone() for k in KEYS])
    return recs


@pytest.mark.parametrize("B", [1, 5])
def test_track_step_is_crop_u8_forward_u8_and_the_tail(B):
    """vt_track_step == vt_crop_u8(out_size 384) + vt_forward_u8(z = None) + vt_update_state_record, bit for bit: records, states, resize
    factors, the 1152-byte-row patch in the workspace, maps and boxes."""
    import torch
    m = _model(8, 26, depth=2)
    res = {mode: _steps(m, B, mode) for mode in ("step", "calls")}
    for a, b in zip(res["step"], res["calls"]):
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(ta, tb), i
    assert torch.isfinite(res["step"][-1][0]).all() and not torch.equal(res["step"][0][1], res["step"][1][1])
    assert torch.equal(res["step"][0][0][:, :4], res["step"][0][1])


def test_chained_step_equals_the_one_chain_step(monkeypatch):
    """B = 64 is the smallest batch whose step runs as two chains (fork_join over vb::Slice; VT_GRAPH_CHAINS is read at model creation): it
    equals the VT_GRAPH_CHAINS=1 step of a second model on the same weights, bit for bit, and the stage composition."""
    import torch
    from vittracker_amd import native
    B = 64
    two = _model(B, 26, depth=2)
    monkeypatch.setenv("VT_GRAPH_CHAINS", "1")
    one = native.Model(TZ, TX, channels=768, heads=12, depth=2, head_channels=256, max_batch=B)
    one.load_state_dict(sd384(26, 2))
    monkeypatch.delenv("VT_GRAPH_CHAINS")
    a, b, c = _steps(two, B, "step"), _steps(one, B, "step"), _steps(two, B, "calls")
    for other in (b, c):
        for sa, sb in zip(a, other):
            for i, (ta, tb) in enumerate(zip(sa, sb)):
                assert torch.equal(ta, tb), i
    assert torch.isfinite(a[-1][0]).all()


def _params():
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters("vitb_384")
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    return p


def test_batched_tracker_and_plugin_on_vitb_384():
    """No tracked sequence of the reference keeps all eight Hann margins above 0.03 at 24 x 24 within 40 seeds (make_golden_vitb384.py), so
    there is no tracking fixture: the tracker is held by exactness.  BatchedVitTracker on vitb_384 (B = 2) and the ostrack plugin give, per
    frame, exactly the record the stage composition gives: crop(192, factor 2.0) + set_template, then crop_u8(384, factor 5.0) +
    forward_u8(None) + update_state_record on a model with the same weights."""
    import torch
    from vittracker_amd import native
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.model_vitb import OSTrack as Net
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    sd = sd384(116)
    seqs = [synthetic_sequence(f"s{q}", 4, seed=1000 * 116 + q) for q in range(2)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]
    fh, fw, _ = seqs[0].frames[0].shape
    assert all(s.frames[0].shape == (fh, fw, 3) for s in seqs)
    # the stage composition, one sequence at a time
    m = _model(3, 116)
    want = []
    for s, b in zip(seqs, box0):
        states = torch.tensor([b], dtype=torch.float64, device="cuda")
        z, rf = m.crop(torch.from_numpy(s.frames[0][None]).cuda(), states, 2.0, TZ, MEAN, STD)
        m.set_template(z)
        out, rec = native.Outputs(1, F, "cuda"), torch.zeros(1, 5, dtype=torch.float64, device="cuda")
        patch = torch.empty(1, TX, TX, 3, dtype=torch.uint8, device="cuda")
        recs = []
        for t in range(1, 4):
            m.crop_u8(torch.from_numpy(s.frames[t][None]).cuda(), states, 5.0, TX, out=patch, resize_factor=rf)
            m.forward_u8(None, patch, out=out)
            m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, TX, fh, fw, margin=10)
            torch.cuda.synchronize()
            recs.append(rec.cpu().numpy()[0].copy())
        want.append(recs)
    bt = BatchedVitTracker(_params(), 2)
    assert isinstance(bt.net, Net)
    bt.net.load_state_dict(sd, strict=False)
    bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
    for t in range(1, 4):
        rec = bt.track_record(np.stack([s.frames[t] for s in seqs]))
        for q in range(2):
            assert np.array_equal(rec[q], want[q][t - 1]), (t, q, rec[q], want[q][t - 1])
    plugin_mod._PIPELINES.clear()
    tr = OSTrack(_params(), "synthetic")
    tr.network.load_state_dict(sd, strict=False)
    tr.initialize(seqs[0].frames[0], {"init_bbox": box0[0]})
    first = tr.track(seqs[0].frames[1])
    assert first["target_bbox"] == want[0][0][:4].tolist() and first["confidence"] == float(np.float32(want[0][0][4]))
    second = tr.track(seqs[0].frames[2])
    assert second["target_bbox"] == want[0][1][:4].tolist()


def test_a_nan_neighbour_frame_does_not_reach_a_frame():
    """The last key chunk of frame 0 reads 16 K rows and, in its last feature row, 16 V^T elements of frame 1.  The kernel masks those
    scores and zeroes those V^T columns in registers, so frame 0 of a batch whose frame 1 is all NaN equals frame 0 run alone, bit for
    bit (depth 2; frame 1's own outputs are not looked at)."""
    import torch
    m = _model(8, 26, depth=2)
    zd, xd = _inputs(11, 2)
    alone = _clone(m.forward(zd[:1].contiguous(), xd[:1].contiguous()))
    zn, xn = zd.clone(), xd.clone()
    zn[1], xn[1] = float("nan"), float("nan")
    both = m.forward(zn, xn)
    assert torch.isfinite(alone.score_map).all()
    for k in ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf"):
        assert torch.equal(getattr(both, k)[0], getattr(alone, k)[0]), k
