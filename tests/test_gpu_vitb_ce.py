"""GPU: OSTrack candidate elimination on the ViT-Base path by key masking (vb_ce.h, vbs::attn_stream_masked_kernel).

The device ranks bf16 rows; neighbouring scores lie 1e-6 apart, so its keep sets cannot be compared token for token with an fp32
reference's.  What is held instead (tests/ce_budget.py holds the truth, the oracle and the band):

  1  test_score_and_selection   the score alone -- a depth-1 model, CE_LOC [0], the regime's tokens fed to blocks(): the device score
                                against the fp64 truth within FACTORS["attn"] (1.65) x E_o, E_o the bf16 oracle's own max error on that
                                input; CTR_POINT, CTR_REC and ALL; plain and peaked; 320 and 720 tokens.
  2  (the same runs)            the selection: exactly the stage's count is kept; every token whose truth score lies above the band is
                                kept and none below it (the band: 2 x 1.65 x E_o either side of the midpoint between the count-th and
                                (count + 1)-th truth scores), on the cases whose inputs keep the band small (ce_budget.BAND_CASES;
                                tests/test_vitb_ce_host.py checks that on the CPU).
  3  test_masked_attention      the masked attention alone -- a depth-2 attn_only model, CE_LOC [0]: resid(2 blocks) - resid(1 block)
                                on the kept rows against the truth under the DEVICE's keep set, bb.judge at FACTORS["attn"]; plain,
                                peaked, last_keys (masked and partial chunks meet), ramp_up; 320 and 720.
  4  test_whole_model           every fixture through forward, forward_u8 where the fixture has a uint8 input, and build_ostrack(cfg):
                                against tests/vitb_ce_oracle.py FORCED to the device's keep sets, maps within TOL_MAP and boxes within
                                TOL_BOX of tests/test_gpu_vitb.py (boxes only for samples whose forced-oracle top-2 margin exceeds 0.03;
                                at least one per fixture must qualify); removed rows of feat exactly 0; stage 1's keep set against the
                                fixture's recorded scores outside the band; later stages nested and of the exact counts.
  5  plumbing                   eager == captured == second replay; B = 66 two chains == one chain (VT_GRAPH_CHAINS=1 in a child process);
                                track_step == crop_u8 -> forward_u8 -> update_state_record; ratios all 1.0 == the plain model; the
                                evaluation harness on the published YAML (result files and their rows, not the exit status); the
                                BatchedVitTracker and the ostrack plugin built from the CE parameters (ce_result shows 256 - 89 removed,
                                every slot == a solo tracker, != the plain YAML's records).  All bit for bit, outputs and ce_result.
  6  ties, ALL on the MFMA      identical search tokens score equal bit for bit and the lower index wins the tie at the cut (plain and
                                MFMA score kernel); CE_TEMPLATE_RANGE ALL (vbc::ce_score_all_kernel) against the plain loop
                                (VB_CE_SCORE_PLAIN=1) within 64 f32 ulps of the largest score, under a second stage's bitmap too."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_budget as bb
import ce_budget as cb
import vbce_cases as vc
from conftest import REPO

pytestmark = pytest.mark.gpu

TOL_MAP = {"score_map": 2.2e-2, "size_map": 2.2e-2, "offset_map": 4.4e-2}      # tests/test_gpu_vitb.py
TOL_BOX = 9e-3
MARGIN = 0.03
# test 4's stage-1 band has to bind at least half of every frame's candidates.  Looser than test 2's BAND_CAP (0.25, which the issue sets for
# inputs chosen to meet it): the fixtures' inputs are fixed by the margin search, and their E_o includes three blocks of bf16 error.
STAGE1_BAND_CAP = 0.5
KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _model(L_or_sizes, depth, sd, B, loc, ratio, rows=None):
    from vittracker_amd import native
    tz, tx = bb.SIZES[L_or_sizes] if isinstance(L_or_sizes, int) else L_or_sizes
    m = native.Model(tz, tx, channels=768, heads=12, depth=depth, head_channels=256, max_batch=B)
    m.load_state_dict(sd)
    if loc is not None:
        m.set_candidate_elimination(loc, ratio, rows)
    return m


def _keep_sets(removed, n):
    """Per stage the (B, count) ascending global indices still present after it, from removed_stage (B, Lx)."""
    out = []
    for k in range(n):
        here = (removed == 0) | (removed > k + 1)
        cnt = here.sum(1)
        assert (cnt == cnt[0]).all(), cnt
        out.append(np.stack([np.flatnonzero(r) for r in here]))
    return out


# ----------------------------------------------------------------------------------------------------- 1, 2: score and selection
@pytest.mark.parametrize("trange", cb.RANGES)
@pytest.mark.parametrize("L", [320, 720])
@pytest.mark.parametrize("name", cb.SCORE_REGIMES)
def test_score_and_selection(name, L, trange):
    import torch
    r = cb.score_refs(name, L)
    ref, count, lz = r[trange], r["count"], r["lz"]
    m = _model(L, 1, r["sd"], cb.SCORE_B, [0], [cb.KEEP_RATIO], cb.range_rows(trange, L))
    try:
        assert m.ce_keep == [count]
        m.blocks(torch.from_numpy(r["X"]).cuda(), nblocks=1)
        removed, scores = m.ce_result(cb.SCORE_B)
        removed, got = removed.cpu().numpy(), scores.cpu().numpy()[0].astype(np.float64)
    finally:
        m.close()
    assert np.isfinite(got).all()
    err, e_o = float(np.abs(got - ref["truth"]).max()), ref["e_o"]
    print(f"score {name} {L} {trange}: device err {err:.3e}, oracle err E_o {e_o:.3e}, x{err / e_o:.2f} (bound x{cb.FACTOR}); "
          f"device - oracle {np.abs(got - ref['oracle']).max():.3e}")
    assert err <= cb.FACTOR * e_o, (err, e_o)
    kept = removed == 0
    assert set(np.unique(removed)) <= {0, 1} and (kept.sum(1) == count).all(), kept.sum(1)
    must_keep, must_drop, share = cb.band(ref["truth"], count, e_o)
    wrong = int((must_keep & ~kept).sum() + (must_drop & kept).sum())
    print(f"selection {name} {L} {trange}: band share {np.round(share, 3)}, outside the band and on the wrong side: {wrong}")
    if (name, L, trange) in cb.BAND_CASES:
        assert max(share) <= cb.BAND_CAP
        assert not (must_keep & ~kept).any(), "a token above the band was removed"
        assert not (must_drop & kept).any(), "a token below the band was kept"


# ----------------------------------------------------------------------------------------------------- 3: masked attention alone
_ATTN_SD = {}


@pytest.mark.parametrize("L", [320, 720])
@pytest.mark.parametrize("name", ["plain", "peaked", "last_keys", "ramp_up"])
def test_masked_attention(name, L):
    import torch
    B = 2
    if (name, L) not in _ATTN_SD:
        sd, X = bb.regime(name, L, B=B, depth=2)
        _ATTN_SD[(name, L)] = (bb.attn_only(bb.attn_only(sd, 0), 1), X)
    sd, X = _ATTN_SD[(name, L)]
    lz = bb.GEOS[L][0]
    m = _model(L, 2, sd, B, [0], [cb.KEEP_RATIO])      # ALL rows: the keep set is the device's own, whatever it is
    try:
        x = torch.from_numpy(X).cuda()
        r1 = m.blocks(x, nblocks=1, want_resid=True)[1].cpu().numpy().astype(np.float64)
        rem1 = m.ce_result(B)[0].cpu().numpy()
        r2 = m.blocks(x, nblocks=2, want_resid=True)[1].cpu().numpy().astype(np.float64)
        rem2 = m.ce_result(B)[0].cpu().numpy()
    finally:
        m.close()
    assert np.array_equal(rem1, rem2) and np.isfinite(r1).all() and np.isfinite(r2).all()
    keep = _keep_sets(rem2, 1)[0]
    assert keep.shape[1] == m.ce_keep[0]
    present = cb.present_mask(L, lz, keep)
    # block 1 from the device's own residual after block 0 (f32 values): only its attention is judged.  The bf16 copy block 1 reads was
    # written by block 0's fc2 GEMM, centred on the mean ln_finalize found after proj: the rows' mean (fc2 adds zero in an attn_only block)
    truth = cb.masked_attention(*bb.qkv(sd, r1, 1, "truth"), present, "truth")
    oracle = cb.masked_attention(*bb.qkv(sd, r1, 1, "bf16", centre=r1.mean(-1)), present, "bf16", chunk=bb.KC)
    got, at = r2 - r1, r1 + truth
    res = bb.judge("attn", cb.kept_rows(got, truth, present), truth, cb.kept_rows(oracle, truth, present), at=at)
    print(f"masked {name} {L}", bb.fmt(res))
    assert res["finite"] and res["ok"], bb.fmt(res)
    if name == "plain":      # the test sees the mask: the UNMASKED oracle in the device's place does not pass (30 % of a flat softmax's keys)
        nomask = bb.attention(*bb.qkv(sd, r1, 1, "bf16", centre=r1.mean(-1)), "bf16", chunk=bb.KC)
        assert not bb.judge("attn", cb.kept_rows(nomask, truth, present), truth, cb.kept_rows(oracle, truth, present), at=at)["ok"]


# ----------------------------------------------------------------------------------------------------- 4: whole model
def _hann_boxes(orc, o):
    import torch
    from vittracker_amd.host_ops import hann2d
    F = orc.feat_sz
    win = hann2d((F, F))
    with torch.no_grad():
        return orc.box_head.cal_bbox(win * o["score_map"], o["size_map"], o["offset_map"]).numpy(), vc.top2((win * o["score_map"]).numpy())


def _against_forced_oracle(c, out, removed, tag, x=None):
    """Maps within TOL_MAP, boxes within TOL_BOX where the forced oracle's margin allows, the stage structure.  -> qualifying samples."""
    n, B = c["n"], c["B"]
    keep = _keep_sets(removed, n)
    counts = [c["g"][f"keep{k}"].shape[1] for k in range(n)]
    assert [k.shape[1] for k in keep] == counts, (tag, [k.shape[1] for k in keep], counts)
    for k in range(1, n):      # nested: removed stays removed
        for b in range(B):
            assert set(keep[k][b]) <= set(keep[k - 1][b]), (tag, k, b)
    o = vc.oracle_run(c, forced=keep, x=x)
    for key, tol in TOL_MAP.items():
        err = np.abs(getattr(out, key).cpu().numpy() - o[key].numpy()).max()
        print(f"{tag} {key}: max err {err:.3e} (tol {tol})")
        assert err <= tol, (tag, key, err)
    raw_ok = vc.top2(o["score_map"].numpy()) > MARGIN
    hb, hm = _hann_boxes(vc.oracle_model(c), o)
    hann_ok = hm > MARGIN
    print(f"{tag}: forced-oracle margins raw {np.round(vc.top2(o['score_map'].numpy()), 4)} hann {np.round(hm, 4)}")
    assert raw_ok.any() or hann_ok.any(), f"{tag}: inconclusive, no sample's forced-oracle margin exceeds {MARGIN}"
    pb = out.pred_boxes.cpu().numpy()
    for b in np.flatnonzero(raw_ok):
        np.testing.assert_allclose(pb[b], o["pred_boxes"].numpy()[b, 0], atol=TOL_BOX, rtol=0, err_msg=f"{tag} pred_boxes {b}")
    for b in np.flatnonzero(hann_ok):
        np.testing.assert_allclose(out.hann_boxes.cpu().numpy()[b], hb[b], atol=TOL_BOX, rtol=0, err_msg=f"{tag} hann_boxes {b}")
    return int(raw_ok.sum() + hann_ok.sum())


@pytest.mark.parametrize("path", vc.files(), ids=vc.ids)
def test_whole_model(path):
    import torch
    from vittracker_amd import config
    from vittracker_amd.model_vitb import build_ostrack, ce_template_rows
    c = vc.load(path)
    g, B, n, lz, lx = c["g"], c["B"], c["n"], c["lz"], c["lx"]
    rows = ce_template_rows(c["range"], c["tz"] // 16)
    m = _model((c["tz"], c["tx"]), c["depth"], c["sd"], B, c["loc"], c["ratio"], rows)
    try:
        zd, xd = torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["x"]).cuda()
        out = m.forward(zd, xd)
        removed = m.ce_result(B)[0].cpu().numpy()
        _against_forced_oracle(c, out, removed, "forward")
        if c["patches"] is not None:
            out8 = m.forward_u8(zd, torch.from_numpy(c["patches"]).cuda())
            _against_forced_oracle(c, out8, m.ce_result(B)[0].cpu().numpy(), "forward_u8")
        # the stages from the fp32 oracle's tokens: feat of removed tokens is exactly 0, and stage 1 against the fixture's scores
        orc, acts = vc.oracle_model(c), {}
        with torch.no_grad():
            orc(torch.from_numpy(c["z"]), torch.from_numpy(c["x"]), acts)
        tokens = acts["tokens"].numpy()
        feat = m.blocks(torch.from_numpy(tokens).cuda()).cpu().numpy()
        rem_b, sc_b = m.ce_result(B)
        rem_b, sc_b = rem_b.cpu().numpy(), sc_b.cpu().numpy()
    finally:
        m.close()
    assert (feat[rem_b != 0] == 0).all() and (np.abs(feat[rem_b == 0]).max(-1) > 0).all()
    for k in range(n):      # a stage's scores are NaN exactly for the tokens removed before it
        assert np.array_equal(np.isnan(sc_b[k]), (rem_b != 0) & (rem_b <= k)), k
    # stage 1 against the fixture's recorded scores: E_o = the max error of the bf16-mirroring chain up to the stage's block (bb.run from
    # the same fp32 tokens, then the score on bf16 q | k; the centring of that block's bf16 copy approximated by the rows' own mean)
    L, loc0, count = lz + lx, c["loc"][0], g["keep0"].shape[1]
    xin = tokens if loc0 == 0 else bb.run(c["sd"], tokens, loc0, "bf16", chunk=bb.KC if L == 720 else None)[0][-1]
    qo, ko, _ = bb.qkv(c["sd"], xin, loc0, "bf16", centre=None if loc0 == 0 else xin.mean(-1))
    mask = None if rows is None else np.asarray(rows)
    e_o = float(np.abs(cb.score(qo, ko, lz, mask) - g["scores0"]).max())
    must_keep, must_drop, share = cb.band(g["scores0"].astype(np.float64), count, e_o)
    kept1 = (rem_b == 0) | (rem_b > 1)
    dev_err = float(np.abs(sc_b[0] - g["scores0"]).max())
    print(f"stage 1: E_o {e_o:.3e}, device score err {dev_err:.3e} (x{dev_err / e_o:.2f}), band share {np.round(share, 3)}, "
          f"agrees with the fixture's keep set on {[int(np.isin(np.flatnonzero(kept1[b]), g['keep0'][b]).sum()) for b in range(B)]} of {count}")
    # the band must bind: at most STAGE1_BAND_CAP of a frame's candidates inside it (a property of the fixture and the CPU oracle alone;
    # the fixtures measure 0.02-0.32); and the device's score is held to the same FACTOR as in test 1
    assert max(share) <= STAGE1_BAND_CAP, share
    assert dev_err <= cb.FACTOR * e_o, (dev_err, e_o)
    assert not (must_keep & ~kept1).any() and not (must_drop & kept1).any()
    # the model-level surface
    cfg = config.fresh_cfg()
    config.update_config_from_file(os.path.join(REPO, "experiments/ostrack", "vitb_384.yaml" if c["tx"] == 384 else "vitb_256.yaml"), cfg)
    bbc = cfg.MODEL.BACKBONE
    bbc.TYPE, bbc.CE_LOC, bbc.CE_KEEP_RATIO, bbc.CE_TEMPLATE_RANGE = "vit_base_patch16_224_ce", c["loc"], c["ratio"], c["range"]
    from vittracker_amd.model_vitb import OSTrack
    net = OSTrack(cfg, depth=c["depth"], max_batch=B) if c["depth"] != 12 else build_ostrack(cfg, training=False, max_batch=B)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c["sd"].items()}, strict=False)
    net = net.cuda().eval()
    full = torch.tensor([True] * lz if rows is None else rows).repeat(B, 1)
    o2 = net(template=zd, search=xd, ce_template_mask=full)
    for key in ("score_map", "size_map", "offset_map"):
        assert torch.equal(o2[key], getattr(out, key)), key
    assert torch.equal(o2["pred_boxes"][:, 0], out.pred_boxes)
    ri = o2["removed_indexes_s"]
    keep = _keep_sets(removed, n)
    prev = np.tile(np.arange(lx), (B, 1))
    assert len(ri) == n
    for k in range(n):
        assert ri[k].dtype == torch.int64
        want = np.stack([np.setdiff1d(prev[b], keep[k][b]) for b in range(B)])
        assert np.array_equal(ri[k].cpu().numpy(), want), k
        prev = keep[k]
    with pytest.raises(ValueError):
        net(template=zd, search=xd, ce_template_mask=~full)
    with pytest.raises(ValueError):
        net(template=zd, search=xd, ce_template_mask=full[:, :-1])
    with pytest.raises(NotImplementedError):
        net(template=zd, search=xd, ce_keep_rate=0.7)
    net._native().close()


# ----------------------------------------------------------------------------------------------------- 5: plumbing
def _published(B, depth=12, ratio=(0.7, 0.7, 0.7), loc=(3, 6, 9), seed=26):
    from vittracker_amd import synth
    from vittracker_amd.model_vitb import ce_template_rows
    sd = synth.synth_vitb_state_dict(seed, depth=depth)
    return _model(320, depth, sd, B, list(loc) if loc else None, list(ratio), ce_template_rows("CTR_POINT", 8) if loc else None), sd


def _snap(out, m, B):
    import torch
    torch.cuda.synchronize()
    r, s = m.ce_result(B)
    return [getattr(out, k).clone() for k in KEYS] + [r.clone(), s.clone()]


def _equal(a, b):
    import torch
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(torch.nan_to_num(x.float(), nan=-7.0), torch.nan_to_num(y.float(), nan=-7.0)), i


def test_eager_equals_captured_equals_second_replay():
    import torch
    from vittracker_amd import synth
    B = 3
    m, _ = _published(B)
    z, x = synth.synth_inputs(5, B, 128, 256)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    eager = _snap(m.forward(zd, xd), m, B)
    assert (eager[6] != 0).sum().item() == B * (256 - 89) and torch.isfinite(eager[0]).all()
    graph, out = m.capture(zd, xd)
    with pytest.raises(Exception, match="before capturing"):
        m.set_candidate_elimination([3], [0.5])
    m.forward(zd.flip(0).contiguous(), xd.flip(0).contiguous())      # something else in the stage buffers
    graph.launch()
    first = _snap(out, m, B)
    graph.launch()
    second = _snap(out, m, B)
    _equal(eager, first)
    _equal(eager, second)
    del graph
    m.close()


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import test_gpu_vitb_ce as T
res = T._chains_run()
np.savez(sys.argv[1], **{str(i): t.cpu().numpy() for i, t in enumerate(res)})
print("CHILD-OK")
"""


def _chains_run():
    """B = 66, depth 3, CE_LOC [0, 1]: forward_u8 on the cached template (two chains from 64 frames up unless VT_GRAPH_CHAINS=1)."""
    import torch
    from vittracker_amd import native, synth
    B = 66
    m, _ = _published(B, depth=3, ratio=(0.7, 0.7), loc=(0, 1))
    m.set_template(torch.from_numpy(synth.synth_inputs(11, B, 128, 256)[0]).cuda())
    out = native.Outputs(B, 16, "cuda")
    m.forward_u8(None, torch.from_numpy(synth.synth_patches(11, B, 256)).cuda(), out=out)
    res = _snap(out, m, B)
    m.close()
    return res


def test_two_chains_equal_one_chain(tmp_path):
    two = _chains_run()
    assert (two[6] != 0).sum().item() == 66 * (256 - 126)
    path = str(tmp_path / "one_chain.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % (REPO, os.path.join(REPO, "tests")), path], env=dict(os.environ, VT_GRAPH_CHAINS="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    one = np.load(path)
    for i, t in enumerate(two):
        assert np.array_equal(one[str(i)], t.cpu().numpy(), equal_nan=True), i


def test_track_step_is_crop_u8_forward_u8_and_the_tail_with_ce():
    import torch
    from vittracker_amd import native
    B, H, W = 3, 120, 160
    m, _ = _published(B)
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([[30 + b, 20 + b, 30 + b, 24 + b] for b in range(B)]).astype(np.float64)
    res = {}
    for mode in ("step", "calls"):
        states = torch.from_numpy(boxes).cuda()
        z, rf = m.crop(frames[0], states, 2.0, 128, MEAN, STD)
        m.set_template(z)
        x, out = torch.empty(B, 3, 256, 256, device="cuda"), native.Outputs(B, 16, "cuda")
        rec, patch = torch.zeros(B, 5, dtype=torch.float64, device="cuda"), torch.empty(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        got = []
        for f in (1, 2):
            if mode == "step":
                m.track_step(frames[f], states, 4.0, MEAN, STD, x, rf, out, record=rec)
            else:
                m.crop_u8(frames[f], states, 4.0, 256, out=patch, resize_factor=rf)
                m.forward_u8(None, patch, out=out)
                m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, 256, H, W, margin=10)
            got.append(_snap(out, m, B) + [rec.clone(), states.clone()])
        res[mode] = got
    m.close()
    for a, b in zip(res["step"], res["calls"]):
        _equal(a, b)
    assert (res["step"][1][6] != 0).sum().item() == B * (256 - 89)


def test_ratios_of_one_are_the_plain_model():
    import torch
    from vittracker_amd import synth
    B = 2
    z, x = synth.synth_inputs(6, B, 128, 256)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    ce, _ = _published(B, ratio=(1.0, 1.0, 1.0))
    plain, _ = _published(B, loc=None)
    a, b = ce.forward(zd, xd), plain.forward(zd, xd)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    removed, scores = ce.ce_result(B)
    assert not removed.any() and torch.isnan(scores).all()
    real, _ = _published(B)
    c = real.forward(zd, xd)
    assert not torch.equal(c.score_map, b.score_map)
    from vittracker_amd import native
    with pytest.raises(native.VtError, match="set_candidate_elimination"):
        plain.ce_result(B)
    for bad in (([12], [0.7]), ([0] * 13, [0.7] * 13)):
        with pytest.raises(native.VtError):
            plain.set_candidate_elimination(*bad)
    with pytest.raises(native.VtError, match="no template row"):
        plain.set_candidate_elimination([3], [0.7], [False] * 64)
    for mm in (ce, plain, real):
        mm.close()


@pytest.mark.parametrize("extra", [[], ["--batch", "2"]], ids=["plugin", "batch2"])
def test_harness_runs_the_published_yaml(extra, tmp_path):
    """tracking/test.py on the published YAML.  The harness prints and skips a sequence or group that raises (evaluation/running.py), so the
    exit status says nothing: every sequence's result file must be there with one row per frame, and no line of the output may be an error."""
    import glob
    env = dict(os.environ, VITTRACK_SAVE_DIR=str(tmp_path), VITTRACK_PRJ_DIR=REPO)
    p = subprocess.run([sys.executable, os.path.join(REPO, "tracking", "test.py"), "ostrack", "vitb_256_mae_ce_32x4_ep300", "--dataset_name", "synthetic:2x4",
                        "--synthetic_weights"] + extra, env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    boxes = sorted(f for f in glob.glob(os.path.join(str(tmp_path), "**", "*.txt"), recursive=True)
                   if not f.endswith(("_time.txt", "_all_boxes.txt", "_all_scores.txt")))
    assert len(boxes) == 2 and all("vitb_256_mae_ce_32x4_ep300" in f for f in boxes), (boxes, p.stdout[-2000:])
    from vittracker_amd.evaluation.data import get_dataset
    frames = {s.name: len(s.frames) for s in get_dataset("synthetic:2x4")}      # ragged: 4 and 6 frames
    assert sorted(os.path.basename(f)[:-4] for f in boxes) == sorted(frames)
    for f in boxes:
        rows = np.loadtxt(f, ndmin=2)
        assert rows.shape == (frames[os.path.basename(f)[:-4]], 4) and np.isfinite(rows).all() and (rows[:, 2:] > 0).all(), (f, rows)
    for word in ("Error", "error", "Traceback", "not implemented", "NotImplemented", "failed"):
        assert word not in p.stdout and word not in p.stderr, (word, p.stdout[-2000:] + p.stderr[-2000:])
    assert p.stdout.count("FPS:") >= 2 and "FPS: -1" not in p.stdout, p.stdout[-2000:]


def _ce_params(name="vitb_256_mae_ce_32x4_ep300"):
    from vittracker_amd.parameter import ostrack as P
    os.environ["VITTRACK_PRJ_DIR"] = REPO
    p = P.parameters(name)
    p.allow_synthetic_weights = True
    p.checkpoint = None
    p.host_crop = False
    return p


def test_batched_tracker_and_plugin_run_with_ce():
    """The tracker front ends built from the CE parameters really run CE: after a step of BatchedVitTracker its native model reports
    256 - 89 removed tokens per frame; every slot of a B = 2 run equals a solo B = 1 tracker bit for bit, and so does the plugin's track();
    and the records differ from the plain YAML's on the same weights."""
    import torch
    from vittracker_amd import synth
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.model_vitb import OSTrack as Net
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    sd = synth.synth_vitb_state_dict(75)
    seqs = [synthetic_sequence(f"s{q}", 4, seed=75000 + q) for q in range(2)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]

    def solo_records(params):
        solo = BatchedVitTracker(params, 1)
        assert isinstance(solo.net, Net)
        solo.net.load_state_dict(sd, strict=False)
        out = []
        for s, b in zip(seqs, box0):
            solo.initialize(s.frames[0][None], [b])
            out.append([solo.track_record(s.frames[t][None])[0] for t in range(1, 4)])
        return solo, out
    solo, want = solo_records(_ce_params())
    assert solo.net.ce_loc == [3, 6, 9]
    removed, scores = solo.net._native().ce_result(1)
    assert (removed != 0).sum().item() == 256 - 89 and [(removed == k).sum().item() for k in (1, 2, 3)] == [76, 54, 37]
    assert torch.isfinite(scores[0]).all()
    _, plain = solo_records(_ce_params("vitb_256"))
    assert not np.array_equal(np.asarray(want), np.asarray(plain)), "the CE tracker gives the plain tracker's records"
    bt = BatchedVitTracker(_ce_params(), 2)
    bt.net.load_state_dict(sd, strict=False)
    bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
    for t in range(1, 4):
        rec = bt.track_record(np.stack([s.frames[t] for s in seqs]))
        for q in range(2):
            assert np.array_equal(rec[q], want[q][t - 1]), (t, q)
    removed = bt.net._native().ce_result(2)[0]
    assert ((removed != 0).sum(1) == 256 - 89).all()
    plugin_mod._PIPELINES.clear()
    tr = OSTrack(_ce_params(), "synthetic")
    tr.network.load_state_dict(sd, strict=False)
    tr.initialize(seqs[0].frames[0], {"init_bbox": box0[0]})
    first = tr.track(seqs[0].frames[1])
    assert first["target_bbox"] == want[0][0][:4].tolist() and first["confidence"] == float(np.float32(want[0][0][4]))
    plugin_mod._PIPELINES.clear()


# ----------------------------------------------------------------------------------------------------- ties, and the MFMA form of ALL
@pytest.mark.parametrize("trange", ["CTR_POINT", "ALL"])
def test_equal_scores_go_to_the_lower_index(trange):
    """Search tokens 2 i and 2 i + 1 are made identical, so their k rows and their scores are equal bit for bit; the stage keeps an ODD
    count (179), so the cut splits one pair: the lower index of a pair is never removed while the higher is kept, and exactly one pair is
    split.  CTR_POINT runs the plain score kernel, ALL the MFMA one."""
    import torch
    r = cb.score_refs("plain", 320)
    lz = r["lz"]
    X = r["X"].copy()
    X[:, lz + 1::2] = X[:, lz:-1:2]
    m = _model(320, 1, r["sd"], cb.SCORE_B, [0], [0.699], cb.range_rows(trange, 320))
    try:
        assert m.ce_keep == [179]
        m.blocks(torch.from_numpy(X).cuda(), nblocks=1)
        removed, scores = m.ce_result(cb.SCORE_B)
        kept, s = removed.cpu().numpy() == 0, scores.cpu().numpy()[0]
    finally:
        m.close()
    assert np.array_equal(s[:, 0::2], s[:, 1::2]), "identical tokens, different scores"
    assert (kept.sum(1) == 179).all()
    lo, hi = kept[:, 0::2], kept[:, 1::2]
    assert not (hi & ~lo).any(), "the higher index of a tie was kept and the lower removed"
    assert ((lo & ~hi).sum(1) == 1).all(), (lo & ~hi).sum(1)


@pytest.mark.parametrize("L", [320, 720])
def test_mfma_score_against_the_plain_loop(L, monkeypatch):
    """CE_TEMPLATE_RANGE ALL runs vbc::ce_score_all_kernel (bf16 MFMA); VB_CE_SCORE_PLAIN=1 sends it through the plain f32 loop instead.
    Both sum the same bf16 products in f32 in different orders: scores within 64 f32 ulps of the largest score (a score is a mean of
    heads x rows softmax weights, each carrying a few ulps of its own), under a second stage's key bitmap too; the keep counts are exact."""
    import torch
    sd, X = bb.regime("plain", L, seed=cb.SEEDS[("plain", L)], B=2, depth=2)
    got = {}
    for plain in ("0", "1"):
        monkeypatch.setenv("VB_CE_SCORE_PLAIN", plain)
        m = _model(L, 2, sd, 2, [0, 1], [0.7, 0.7])
        try:
            m.blocks(torch.from_numpy(X).cuda(), nblocks=2)
            removed, scores = m.ce_result(2)
            got[plain] = (removed.cpu().numpy(), scores.cpu().numpy().astype(np.float64))
        finally:
            m.close()
    (ra, sa), (rb, sb) = got["0"], got["1"]
    lx = L - bb.GEOS[L][0]
    assert [(ra == 0).sum(1).tolist(), (rb == 0).sum(1).tolist()] == [[m.ce_keep[1]] * 2] * 2
    # stage 1 ran on all keys in both runs; stage 2's bitmap is each run's own, so it is compared where both runs kept the token
    tol = 64 * 2.0 ** -23 * float(np.nanmax(sb))
    d1 = np.abs(sa[0] - sb[0]).max()
    both = ~np.isnan(sa[1]) & ~np.isnan(sb[1])
    print(f"mfma vs plain {L}: stage 1 max diff {d1:.3e} (tol {tol:.3e}), stage-1 keep sets differ in {int(((ra == 1) != (rb == 1)).sum())} of {2 * lx}")
    assert d1 <= tol and both.sum() > lx
    if np.array_equal(ra == 1, rb == 1):
        assert np.abs(sa[1] - sb[1])[both].max() <= tol
