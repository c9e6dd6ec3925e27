"""GPU: the compact form of OSTrack candidate elimination on the ViT-Base path (vb_ce.h, vbs::attn_stream_rt_kernel):
behind every stage the kept tokens are gathered into shorter frames and everything behind runs on B x Lp rows.  Same function, same
public results as the masked form (tests/test_gpu_vitb_ce.py, whose helpers, tolerances and constructions are reused here).

  1  test_stage1_is_the_masked_forms   the first removing stage scores and selects before anything moves: ce_result bit-identical between the
                                       forms for one stage, under CTR_POINT (the plain loop) and ALL (the MFMA form); 320 and 720.
     test_stage1_under_the_published_three_stages   stage 1's scores and removed set under the published three stages; 320 and 720.
  2  test_compacted_attention          test_masked_attention's construction in the compact form, the bf16 oracle chunked over the COMPACTED
                                       key order; keep ratios chosen for the tails of the run-time kernel (ce_compact_cases.ATTN_RATIOS).
     test_pad_and_read_past_rows_are_never_used   NaN / stale rows beyond the live ones: the kept rows do not change by a bit.
  3  test_stage2_on_compacted_rows     the score and selection on compacted q | k rows, through the index table; the MFMA form against the
                                       plain loop; ties at stage 2.
  4  test_whole_model                  every fixture against the oracle forced to the device's keep sets: catches a wrong index anywhere in
                                       gather or scatter; and with VB_LN_FOLD=0 / VB_LN_CENTER=0 (the per-row LayerNorms on compacted rows).
  5  plumbing                          eager == captured == replay; two chains == one; track_step == its parts; ratios 1.0 == plain; the
                                       tracker front ends; back to "masked"."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bf16_budget as bb
import ce_budget as cb
import ce_compact_cases as cc
import test_gpu_vitb_ce as T
import vbce_cases as vc
from conftest import REPO

pytestmark = pytest.mark.gpu


def _result(m, B):
    r, s = m.ce_result(B)
    return r.cpu().numpy(), s.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1: stage 1 is the masked form's
@pytest.mark.parametrize("trange", ["CTR_POINT", "ALL"])      # the plain score loop and the MFMA form: one launch choice under both forms
@pytest.mark.parametrize("L", [320, 720])
def test_stage1_is_the_masked_forms(L, trange):
    import torch
    r = cb.score_refs("plain", L)
    x = torch.from_numpy(r["X"]).cuda()
    got = {}
    for form in ("masked", "compact"):
        m = cc.model(L, 1, r["sd"], cb.SCORE_B, [0], [cb.KEEP_RATIO], cb.range_rows(trange, L), form=form)
        try:
            assert m.ce_form == form
            m.blocks(x, nblocks=1)
            got[form] = _result(m, cb.SCORE_B)
        finally:
            m.close()
    assert np.array_equal(got["masked"][0], got["compact"][0]) and np.array_equal(got["masked"][1], got["compact"][1])
    assert ((got["compact"][0] == 0).sum(1) == r["count"]).all()


@pytest.mark.parametrize("L", [320, 720])
def test_stage1_under_the_published_three_stages(L):
    """The published three stages (depth 4: blocks 0, 1, 2): stage 1's scores and its removed set are the masked form's."""
    import torch
    got = {}
    sd, X = bb.regime("plain", L, seed=cb.SEEDS[("plain", L)], B=2, depth=4)
    x = torch.from_numpy(X).cuda()
    for form in ("masked", "compact"):
        m = cc.model(L, 4, sd, 2, [0, 1, 2], [0.7, 0.7, 0.7], cb.range_rows("CTR_POINT", L), form=form)
        try:
            m.blocks(x)
            got[form] = _result(m, 2)
            keep = m.ce_keep
        finally:
            m.close()
    assert np.array_equal(got["masked"][1][0], got["compact"][1][0])
    assert np.array_equal(got["masked"][0] == 1, got["compact"][0] == 1)
    assert [int((got["compact"][0][0] == k).sum()) for k in (0, 1, 2, 3)] == [keep[2], L - bb.GEOS[L][0] - keep[0], keep[0] - keep[1], keep[1] - keep[2]]


# ------------------------------------------------------------------------------------------ 2: compacted attention alone
_ATTN = {}
ATTN_CASES = [(320, r) for r in cc.ATTN_RATIOS] + [(720, 0.7)]


def _attn_case(name, L):
    if (name, L) not in _ATTN:
        sd, X = bb.regime(name, L, B=2, depth=2)
        _ATTN[(name, L)] = (bb.attn_only(bb.attn_only(sd, 0), 1), X)
    return _ATTN[(name, L)]


@pytest.mark.parametrize("L,ratio", ATTN_CASES)
@pytest.mark.parametrize("name", ["plain", "peaked", "last_keys", "ramp_up"])
def test_compacted_attention(name, L, ratio):
    import torch
    from vittracker_amd import native
    B = 2
    sd, X = _attn_case(name, L)
    lz, lx = bb.GEOS[L]
    m = cc.model(L, 2, sd, B, [0], [ratio])
    try:
        x = torch.from_numpy(X).cuda()
        r1 = m.blocks(x, nblocks=1, want_resid=True)[1].cpu().numpy().astype(np.float64)
        rem1 = m.ce_result(B)[0].cpu().numpy()
        r2 = m.blocks(x, nblocks=2, want_resid=True)[1].cpu().numpy().astype(np.float64)
        rem2 = m.ce_result(B)[0].cpu().numpy()
        count = m.ce_keep[0]
    finally:
        m.close()
    assert np.array_equal(rem1, rem2) and np.isfinite(r1).all() and np.isfinite(r2).all()
    keep = T._keep_sets(rem2, 1)[0]
    assert keep.shape[1] == count and native.ce_compact_lengths(lz, lx, [ratio]) == [(lz + count + 15) // 16 * 16]
    if L == 320:
        assert (lz + count, native.ce_compact_lengths(lz, lx, [ratio])[0]) == cc.ATTN_RATIOS[ratio]
    present = cb.present_mask(L, lz, keep)
    assert (r1[~present] == 0).all() and (r2[~present] == 0).all(), "resid_out rows of removed tokens are zeros"
    # block 1 from the device's own residual after block 0 (its kept rows; rows of removed tokens are never read)
    truth = cb.masked_attention(*bb.qkv(sd, r1, 1, "truth"), present, "truth")
    qo, ko, vo_ = bb.qkv(sd, r1, 1, "bf16", centre=r1.mean(-1))
    oracle = cc.compact_attention(qo, ko, vo_, keep, lz, "bf16", chunk=bb.KC)
    got, at = r2 - r1, r1 + truth
    res = bb.judge("attn", cb.kept_rows(got, truth, present), truth, cb.kept_rows(oracle, truth, present), at=at)
    print(f"compact {name} {L} ratio {ratio}", bb.fmt(res))
    assert res["finite"] and res["ok"], bb.fmt(res)
    if name == "plain":      # the test sees the removal: the oracle over ALL keys in the device's place does not pass
        nomask = bb.attention(qo, ko, vo_, "bf16", chunk=bb.KC)
        assert not bb.judge("attn", cb.kept_rows(nomask, truth, present), truth, cb.kept_rows(oracle, truth, present), at=at)["ok"]


@pytest.mark.parametrize("L,ratio", [(320, 0.7), (320, 0.43), (720, 0.7)])
def test_pad_and_read_past_rows_are_never_used(L, ratio):
    """The same two frames before and after a larger batch has left other values -- a NaN frame among them -- in every workspace row
    beyond the two frames' live rows (pad rows, the rows the last key chunk reads past the frame, the third frame's rows at every stride):
    the kept rows, the scores and the features do not change by a bit."""
    import torch
    sd, X = _attn_case("plain", L)
    m = cc.model(L, 2, sd, 3, [0], [ratio])
    try:
        x = torch.from_numpy(X).cuda()

        def run():
            feat, resid = m.blocks(x, nblocks=2, want_resid=True)
            torch.cuda.synchronize()
            return [feat.clone(), resid.clone()] + [t.clone() for t in m.ce_result(2)]
        before = run()
        poison = torch.from_numpy(np.concatenate([X[::-1] * 3.0, np.full_like(X[:1], np.nan)])).cuda()
        m.blocks(poison, nblocks=2)
        after = run()
    finally:
        m.close()
    assert torch.isfinite(before[0]).all() and torch.isfinite(before[1]).all()
    T._equal(before, after)


# ------------------------------------------------------------------------------------------ 3: stage 2 on compacted rows
def _stage2_device(L, trange):
    """The stage-2 model on the device: dense resid after block 0, removed_stage and scores after both stages."""
    import torch
    sd, X0 = cc.stage2_case(L)
    m = cc.model(L, 2, sd, 2, [0, 1], cc.STAGE2_RATIOS, cb.range_rows(trange, L))
    try:
        x = torch.from_numpy(X0).cuda()
        r1 = m.blocks(x, nblocks=1, want_resid=True)[1].cpu().numpy()
        m.blocks(x, nblocks=2)
        removed, scores = _result(m, 2)
        return sd, r1, removed, scores, list(m.ce_keep)
    finally:
        m.close()


@pytest.mark.parametrize("trange", cb.RANGES)
@pytest.mark.parametrize("L", [320, 720])
def test_stage2_on_compacted_rows(L, trange):
    sd, r1, removed, scores, counts = _stage2_device(L, trange)
    lz = bb.GEOS[L][0]
    keep = T._keep_sets(removed, 2)
    assert [k.shape[1] for k in keep] == counts
    for b in range(2):
        assert set(keep[1][b]) <= set(keep[0][b])
    for k in range(2):      # NaN exactly for the tokens removed before the stage
        assert np.array_equal(np.isnan(scores[k]), (removed != 0) & (removed <= k)), k
    ref = cc.stage2_refs(sd, r1, keep[0], lz, cb.range_rows(trange, L), counts[1])
    live = ~np.isnan(ref["truth"])
    assert np.array_equal(live, ~np.isnan(scores[1]))
    err = float(np.abs(scores[1].astype(np.float64) - ref["truth"])[live].max())
    print(f"stage 2 {L} {trange}: device err {err:.3e}, oracle err E_o {ref['e_o']:.3e}, x{err / ref['e_o']:.2f} (bound x{cb.FACTOR}); "
          f"band share {np.round(ref['share'], 3)}")
    assert err <= cb.FACTOR * ref["e_o"], (err, ref["e_o"])
    kept2 = removed == 0
    assert max(ref["share"]) <= cb.BAND_CAP, ref["share"]
    assert not (ref["must_keep"] & ~kept2).any(), "a token above the band was removed"
    assert not (ref["must_drop"] & kept2).any(), "a token below the band was kept"


@pytest.mark.parametrize("L", [320, 720])
def test_stage2_mfma_score_against_the_plain_loop(L, monkeypatch):
    """CE_TEMPLATE_RANGE ALL at stage 2 runs vbc::ce_score_all_rt_kernel; VB_CE_SCORE_PLAIN=1 the plain run-time loop.  As in
    test_gpu_vitb_ce.py: within 64 f32 ulps of the largest score.  Stage 2 is the only place the run-time MFMA kernel runs, so the two
    runs' stage-1 sets must be equal on these inputs (the two stage-1 kernels agree to under 1 ulp of the largest score there) -- were
    they not, the comparison would say nothing, and the test fails."""
    got = {}
    for plain in ("0", "1"):
        monkeypatch.setenv("VB_CE_SCORE_PLAIN", plain)
        _, _, removed, scores, counts = _stage2_device(L, "ALL")
        got[plain] = (removed, scores.astype(np.float64))
    (ra, sa), (rb, sb) = got["0"], got["1"]
    assert [(ra == 0).sum(1).tolist(), (rb == 0).sum(1).tolist()] == [[counts[1]] * 2] * 2
    tol = 64 * 2.0 ** -23 * float(np.nanmax(sb))
    d1 = np.abs(sa[0] - sb[0]).max()
    both = ~np.isnan(sa[1]) & ~np.isnan(sb[1])
    same = np.array_equal(ra == 1, rb == 1)
    print(f"stage-2 mfma vs plain {L}: stage 1 max diff {d1:.3e}, stage-1 sets equal {same}, stage 2 max diff "
          f"{np.abs(sa[1] - sb[1])[both].max():.3e} (tol {tol:.3e})")
    assert d1 <= tol and both.sum() > counts[1]
    assert same, "the two runs' stage-1 keep sets differ: stage 2 compares different candidates"
    assert np.array_equal(np.isnan(sa[1]), np.isnan(sb[1])) and np.abs(sa[1] - sb[1])[both].max() <= tol


@pytest.mark.parametrize("trange", ["CTR_POINT", "ALL"])
def test_equal_scores_go_to_the_lower_global_index_at_stage2(trange):
    """Search tokens 2 i and 2 i + 1 identical: equal scores bit for bit at both stages, pairs removed or kept together but for the one pair an
    odd count splits -- and there the lower GLOBAL index stays, at stage 2 through the index table."""
    sd, X = cc.stage2_case(320)
    X = X.copy()
    X[:, 64 + 1::2] = X[:, 64:-1:2]
    import torch
    m = cc.model(320, 2, sd, 2, [0, 1], [0.699, 0.699], cb.range_rows(trange, 320))
    try:
        assert m.ce_keep == [179, 126]
        m.blocks(torch.from_numpy(X).cuda(), nblocks=2)
        removed, scores = _result(m, 2)
    finally:
        m.close()
    assert np.array_equal(scores[0][:, 0::2], scores[0][:, 1::2]), "identical tokens, different scores at stage 1"
    pair = ~np.isnan(scores[1][:, 0::2]) & ~np.isnan(scores[1][:, 1::2])      # both of a pair still there at stage 2
    assert np.array_equal(scores[1][:, 0::2][pair], scores[1][:, 1::2][pair]) and pair.sum() >= 2 * 89, "identical tokens, different scores at stage 2"
    for k, count in ((1, 179), (2, 126)):
        here = (removed == 0) | (removed > k)
        assert (here.sum(1) == count).all()
        lo, hi = here[:, 0::2], here[:, 1::2]
        assert not (hi & ~lo).any(), f"stage {k}: the higher index of a tie was kept and the lower removed"
    # stage 1 splits one pair (179 is odd); at stage 2 the 126 kept are 63 whole pairs or 62 pairs + the stage-1 single + one split pair
    assert (((removed[:, 0::2] == 0) | (removed[:, 0::2] > 1)) & (removed[:, 1::2] == 1)).sum(1).tolist() == [1, 1]
    # the scores at stage 2 of a pair that stage 1 split: the survivor's is a number, the removed one's NaN
    assert np.isnan(scores[1][removed == 1]).all() and not np.isnan(scores[1][removed != 1]).any()


# ------------------------------------------------------------------------------------------ 4: whole model
@pytest.mark.parametrize("path", vc.files(), ids=vc.ids)
def test_whole_model(path):
    import torch
    from vittracker_amd import config
    from vittracker_amd.model_vitb import OSTrack, build_ostrack, ce_template_rows
    c = vc.load(path)
    B, n, lz, lx = c["B"], c["n"], c["lz"], c["lx"]
    rows = ce_template_rows(c["range"], c["tz"] // 16)
    m = cc.model((c["tz"], c["tx"]), c["depth"], c["sd"], B, c["loc"], c["ratio"], rows)
    try:
        zd, xd = torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["x"]).cuda()
        out = m.forward(zd, xd)
        removed = m.ce_result(B)[0].cpu().numpy()
        T._against_forced_oracle(c, out, removed, "compact forward")
        if c["patches"] is not None:
            out8 = m.forward_u8(zd, torch.from_numpy(c["patches"]).cuda())
            T._against_forced_oracle(c, out8, m.ce_result(B)[0].cpu().numpy(), "compact forward_u8")
        orc, acts = vc.oracle_model(c), {}
        with torch.no_grad():
            orc(torch.from_numpy(c["z"]), torch.from_numpy(c["x"]), acts)
        feat = m.blocks(torch.from_numpy(acts["tokens"].numpy()).cuda()).cpu().numpy()
        rem_b, sc_b = _result(m, B)
    finally:
        m.close()
    assert (feat[rem_b != 0] == 0).all() and (np.abs(feat[rem_b == 0]).max(-1) > 0).all()
    for k in range(n):
        assert np.array_equal(np.isnan(sc_b[k]), (rem_b != 0) & (rem_b <= k)), k
    # the model-level surface
    cfg = config.fresh_cfg()
    config.update_config_from_file(os.path.join(REPO, "experiments/ostrack", "vitb_384.yaml" if c["tx"] == 384 else "vitb_256.yaml"), cfg)
    bbc = cfg.MODEL.BACKBONE
    bbc.TYPE, bbc.CE_LOC, bbc.CE_KEEP_RATIO, bbc.CE_TEMPLATE_RANGE = "vit_base_patch16_224_ce", c["loc"], c["ratio"], c["range"]
    net = OSTrack(cfg, depth=c["depth"], max_batch=B, ce_form="compact") if c["depth"] != 12 else build_ostrack(cfg, training=False, max_batch=B, ce_form="compact")
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c["sd"].items()}, strict=False)
    net = net.cuda().eval()
    o2 = net(template=zd, search=xd)
    assert net._native().ce_form == "compact"
    for key in ("score_map", "size_map", "offset_map"):
        assert torch.equal(o2[key], getattr(out, key)), key
    assert torch.equal(o2["pred_boxes"][:, 0], out.pred_boxes)
    ri, keep, prev = o2["removed_indexes_s"], T._keep_sets(removed, n), np.tile(np.arange(lx), (B, 1))
    assert len(ri) == n
    for k in range(n):
        assert ri[k].dtype == torch.int64
        assert np.array_equal(ri[k].cpu().numpy(), np.stack([np.setdiff1d(prev[b], keep[k][b]) for b in range(B)])), k
        prev = keep[k]
    net._native().close()


@pytest.mark.parametrize("switch", ["VB_LN_FOLD", "VB_LN_CENTER"])
def test_whole_model_with_the_layernorm_switches_off(switch, monkeypatch):
    """VB_LN_FOLD=0: the per-row LayerNorm kernels run on the compacted B x Lp rows; VB_LN_CENTER=0: the proj GEMM behind a gather centres
    nothing.  The smallest fixture against the oracle forced to the device's keep sets, at the same tolerances."""
    import torch
    from vittracker_amd.model_vitb import ce_template_rows
    monkeypatch.setenv(switch, "0")
    c = vc.load([p for p in vc.files() if "d3" in p][0])
    m = cc.model((c["tz"], c["tx"]), c["depth"], c["sd"], c["B"], c["loc"], c["ratio"], ce_template_rows(c["range"], c["tz"] // 16))
    try:
        out = m.forward(torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["x"]).cuda())
        T._against_forced_oracle(c, out, m.ce_result(c["B"])[0].cpu().numpy(), f"compact {switch}=0")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 5: plumbing
def _published(B, depth=12, ratio=(0.7, 0.7, 0.7), loc=(3, 6, 9), seed=26, form="compact"):
    from vittracker_amd import synth
    from vittracker_amd.model_vitb import ce_template_rows
    sd = synth.synth_vitb_state_dict(seed, depth=depth)
    return cc.model(320, depth, sd, B, list(loc) if loc else None, list(ratio), ce_template_rows("CTR_POINT", 8) if loc else None, form=form)


def test_eager_equals_captured_equals_second_replay():
    import torch
    from vittracker_amd import native, synth
    B = 3
    m = _published(B)
    z, x = synth.synth_inputs(5, B, 128, 256)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    eager = T._snap(m.forward(zd, xd), m, B)
    assert (eager[6] != 0).sum().item() == B * (256 - 89) and torch.isfinite(eager[0]).all()
    graph, out = m.capture(zd, xd)
    with pytest.raises(native.VtError, match="before capturing"):
        m.set_candidate_elimination([3], [0.5], form="masked")
    m.forward(zd.flip(0).contiguous(), xd.flip(0).contiguous())      # something else in the stage buffers and index tables
    graph.launch()
    first = T._snap(out, m, B)
    graph.launch()
    second = T._snap(out, m, B)
    T._equal(eager, first)
    T._equal(eager, second)
    del graph
    m.close()


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import test_gpu_vitb_ce_compact as TC
res = TC._chains_run()
np.savez(sys.argv[1], **{str(i): t.cpu().numpy() for i, t in enumerate(res)})
print("CHILD-OK")
"""


def _chains_run():
    """B = 66, depth 4, CE_LOC [0, 1, 2]: forward_u8 on the cached template (two chains from 64 frames up unless VT_GRAPH_CHAINS=1)."""
    import torch
    from vittracker_amd import native, synth
    B = 66
    m = _published(B, depth=4, loc=(0, 1, 2))
    m.set_template(torch.from_numpy(synth.synth_inputs(11, B, 128, 256)[0]).cuda())
    out = native.Outputs(B, 16, "cuda")
    m.forward_u8(None, torch.from_numpy(synth.synth_patches(11, B, 256)).cuda(), out=out)
    res = T._snap(out, m, B)
    m.close()
    return res


def test_two_chains_equal_one_chain(tmp_path):
    two = _chains_run()
    assert (two[6] != 0).sum().item() == 66 * (256 - 89)
    path = str(tmp_path / "one_chain.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % (REPO, os.path.join(REPO, "tests")), path], env=dict(os.environ, VT_GRAPH_CHAINS="1"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    one = np.load(path)
    for i, t in enumerate(two):
        assert np.array_equal(one[str(i)], t.cpu().numpy(), equal_nan=True), i


def test_track_step_is_crop_u8_forward_u8_and_the_tail():
    import torch
    from vittracker_amd import native
    B, H, W = 3, 120, 160
    m = _published(B)
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
    boxes = np.stack([[30 + b, 20 + b, 30 + b, 24 + b] for b in range(B)]).astype(np.float64)
    res = {}
    for mode in ("step", "calls"):
        states = torch.from_numpy(boxes).cuda()
        z, rf = m.crop(frames[0], states, 2.0, 128, T.MEAN, T.STD)
        m.set_template(z)
        x, out = torch.empty(B, 3, 256, 256, device="cuda"), native.Outputs(B, 16, "cuda")
        rec, patch = torch.zeros(B, 5, dtype=torch.float64, device="cuda"), torch.empty(B, 256, 256, 3, dtype=torch.uint8, device="cuda")
        got = []
        for f in (1, 2):
            if mode == "step":
                m.track_step(frames[f], states, 4.0, T.MEAN, T.STD, x, rf, out, record=rec)
            else:
                m.crop_u8(frames[f], states, 4.0, 256, out=patch, resize_factor=rf)
                m.forward_u8(None, patch, out=out)
                m.update_state_record(out.hann_boxes, out.conf, rf, states, rec, 256, H, W, margin=10)
            got.append(T._snap(out, m, B) + [rec.clone(), states.clone()])
        res[mode] = got
    m.close()
    for a, b in zip(res["step"], res["calls"]):
        T._equal(a, b)
    assert (res["step"][1][6] != 0).sum().item() == B * (256 - 89)


def test_ratios_of_one_are_the_plain_model_and_masked_comes_back():
    import torch
    from vittracker_amd import native, synth
    B = 2
    z, x = synth.synth_inputs(6, B, 128, 256)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    ce, plain = _published(B, ratio=(1.0, 1.0, 1.0)), _published(B, loc=None)
    a, b = ce.forward(zd, xd), plain.forward(zd, xd)
    torch.cuda.synchronize()
    for k in T.KEYS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    removed, scores = ce.ce_result(B)
    assert not removed.any() and torch.isnan(scores).all()
    # a model switched back to "masked" reproduces a fresh masked model, and differs from nothing but by rounding from the compact one
    real, masked = _published(B), _published(B, form="masked")
    comp = T._snap(real.forward(zd, xd), real, B)
    assert not torch.equal(comp[0], b.score_map)
    real.set_candidate_elimination([3, 6, 9], [0.7] * 3, [i == 27 for i in range(64)], form="masked")
    assert real.ce_form == "masked"
    T._equal(T._snap(real.forward(zd, xd), real, B), T._snap(masked.forward(zd, xd), masked, B))
    with pytest.raises(native.VtError, match="one of"):
        plain.set_candidate_elimination([3], [0.7], form="dense")
    assert plain._L.vt_set_ce_form(plain._h, 7) == -1 and b"VT_CE_COMPACT" in plain._L.vt_last_error()
    for mm in (ce, plain, real, masked):
        mm.close()
    large = native.Model(128, 256, channels=1024, heads=16, depth=1, head_channels=256, max_batch=1)
    try:
        with pytest.raises(native.VtError, match="ViT-Base"):
            large.set_candidate_elimination([0], [0.7], form="compact")
        assert large._L.vt_set_ce_form(large._h, 1) == -1 and b"ViT-Base" in large._L.vt_last_error()
    finally:
        large.close()


def test_batched_tracker_and_plugin_run_compact(monkeypatch):
    """The tracker front ends built with ce_form = "compact": the native model reports the form and 256 - 89 removed tokens per frame; every
    slot of a B = 2 run equals a solo B = 1 tracker bit for bit, and so does the plugin's track()."""
    import torch
    from vittracker_amd import synth
    from vittracker_amd.batched import BatchedVitTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    from vittracker_amd.tracker import vit_dist as plugin_mod
    from vittracker_amd.tracker.ostrack import OSTrack
    monkeypatch.delenv("VB_CE_FORM", raising=False)
    sd = synth.synth_vitb_state_dict(75)
    seqs = [synthetic_sequence(f"s{q}", 4, seed=75000 + q) for q in range(2)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]

    def params():
        p = T._ce_params()
        p.ce_form = "compact"
        return p
    solo = BatchedVitTracker(params(), 1)
    solo.net.load_state_dict(sd, strict=False)
    assert solo.net.ce_form == "compact" and solo.net._native().ce_form == "compact"
    want = []
    for s, b in zip(seqs, box0):
        solo.initialize(s.frames[0][None], [b])
        want.append([solo.track_record(s.frames[t][None])[0] for t in range(1, 4)])
    removed, scores = solo.net._native().ce_result(1)
    assert (removed != 0).sum().item() == 256 - 89 and [(removed == k).sum().item() for k in (1, 2, 3)] == [76, 54, 37]
    assert torch.isfinite(scores[0]).all()
    bt = BatchedVitTracker(params(), 2)
    bt.net.load_state_dict(sd, strict=False)
    bt.initialize(np.stack([s.frames[0] for s in seqs]), box0)
    for t in range(1, 4):
        rec = bt.track_record(np.stack([s.frames[t] for s in seqs]))
        for q in range(2):
            assert np.array_equal(rec[q], want[q][t - 1]), (t, q)
    assert ((bt.net._native().ce_result(2)[0] != 0).sum(1) == 256 - 89).all()
    plugin_mod._PIPELINES.clear()
    tr = OSTrack(params(), "synthetic")
    assert tr.network.ce_form == "compact"
    tr.network.load_state_dict(sd, strict=False)
    tr.initialize(seqs[0].frames[0], {"init_bbox": box0[0]})
    first = tr.track(seqs[0].frames[1])
    assert first["target_bbox"] == want[0][0][:4].tolist() and first["confidence"] == float(np.float32(want[0][0][4]))
    plugin_mod._PIPELINES.clear()


def test_sharded_tracker_runs_compact(monkeypatch):
    """ShardedBatchedTracker built from parameters with ce_form = "compact": every shard's native model runs the compact form, and every
    sequence's records equal one compact BatchedVitTracker's of all sequences, bit for bit."""
    from vittracker_amd import synth
    from vittracker_amd.batched import BatchedVitTracker, ShardedBatchedTracker
    from vittracker_amd.evaluation.data import synthetic_sequence
    monkeypatch.delenv("VB_CE_FORM", raising=False)
    sd = synth.synth_vitb_state_dict(75)
    seqs = [synthetic_sequence(f"s{q}", 3, seed=75000 + q) for q in range(3)]
    box0 = [list(map(float, s.ground_truth_rect[0])) for s in seqs]
    p = T._ce_params()
    p.ce_form = "compact"

    def boxes(tracker, nets):
        for net in nets:
            net.load_state_dict(sd, strict=False)
        tracker.initialize(np.stack([s.frames[0] for s in seqs]), box0)
        return [np.asarray(tracker.track(np.stack([s.frames[t] for s in seqs]))["target_bbox"]).copy() for t in (1, 2)]
    one = BatchedVitTracker(p, 3)
    want = boxes(one, [one.net])
    sh = ShardedBatchedTracker(p, 3, 2)
    assert sh.sizes == [2, 1] and all(t.net.ce_form == "compact" and t.nat.ce_form == "compact" for t in sh.trackers)
    got = boxes(sh, [t.net for t in sh.trackers])
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    for t in sh.trackers:
        assert ((t.nat.ce_result(t.B)[0] != 0).sum(1) == 256 - 89).all()

