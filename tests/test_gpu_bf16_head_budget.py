"""GPU: the ViT box head (vb::head: feat_to_map_kernel, the conv towers as implicit GEMMs, conv5_kernel) against the fp64 truth, held to a
multiple of the bf16 oracle's own error on the same features (tests/bf16_head_budget.py) -- per map and per (frame, output channel), at
widths 1024 / 768 / 384 / 192, at F = 16 (128 / 256 px, B = 2) and F = 24 (192 / 384 px, B = 3: M = 1728 = 6.75 x 256, tiles straddle frame
boundaries and the last one is partial), on both tile forms:

  default   the automatic choice, at these batches the narrow 128 x 64 tile for conv1 and conv2 (gemm_form's head bit set)
  wide      VB_GEMM_NARROW=0 (read at model creation): conv1 on the 256 x 256 software-pipelined tile at 1024 / 768 / 384 and on the
            256 x 64 two-buffer tile at 192 (27 k-tiles), conv2 on the 256 x 256 tile with three groups (head bit clear)
conv3 / conv4 run the 256 x 64 tile in both.  Models are depth 1 with head_channels = 256; features go straight into ``m.head(feat)``.

  test_head_within_budget[C-F-form-regime]     all four regimes on default, plain and one_token on wide; one_token's nine frames as
                                               launches of B (the last of F = 16 is one frame)
  test_partial_tiles_at_F24[C]                 B = 1: M = 576 = 2.25 x 256 = 4.5 x 128, both forms
  test_head_on_a_frame_slice                   width 768, F = 24: a step of 3 frames captured as two chains, slices [0, 1) and [1, 3) with
                                               Bt = 3 in the tower-major strides, equals the unsliced step's bytes and holds the budget
  test_forward_head_equals_staged_head[C]      forward (the head reads the final-LayerNorm kernel's map) == head(blocks(stem)) (the map
                                               of feat_to_map_kernel), bit for bit on maps and boxes, on a model whose block adds nothing
                                               to the residual stream (``_passthrough``: with a live block the two chains differ in the
                                               BLOCK, by design -- measured: every width's score_map differs)
  test_shrinking_batch_leaves_no_trace         B = 3 edge_hot, then B = 1 one_token on the same model == a fresh model's B = 1

Asserted: finite, and err(kernel) <= FACTORS[map] x err(oracle) + floor for rel-L2 and max-abs, of the map and of every (frame, channel)
slot.  Every case prints its bf16_head_budget.fmt rows (with the worst 8 x 8 tile and the kernel - oracle distance, not asserted).  The
measured table is in bf16_head_budget.FACTORS' comment and NOTES.md."""
import numpy as np
import pytest

import bf16_head_budget as hb

pytestmark = pytest.mark.gpu

WIDTHS = (1024, 768, 384, 192)
FORMS = {"default": None, "wide": "0"}          # VB_GEMM_NARROW at model creation
KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
_REF = {}


def _ref(C, F, name, B=None):
    """CPU references, once per (width, map size, regime, frames): state dict, features, truth, oracle.  One width is kept at a time."""
    B = (9 if name == "one_token" else hb.GEOMS[F][2]) if B is None else B
    key = (C, F, name, B)
    if key not in _REF:
        for k in [k for k in _REF if k[0] != C]:
            del _REF[k]
        sd = hb.state(C, F)
        X = hb.regime(name, B, F, C)
        _REF[key] = {"sd": sd, "X": X, "truth": hb.head(sd, X, "truth"), "oracle": hb.head(sd, X, "bf16")}
    return _REF[key]


def _model(C, F, form, sd, monkeypatch, max_batch, chains=None):
    from vittracker_amd import native
    for k in ("VB_GEMM_NARROW", "VB_GEMM_NARROW_FILL", "VT_GRAPH_CHAINS", "VT_CHAIN_CUS"):
        monkeypatch.delenv(k, raising=False)
    if FORMS[form] is not None:
        monkeypatch.setenv("VB_GEMM_NARROW", FORMS[form])
    if chains is not None:
        monkeypatch.setenv("VT_GRAPH_CHAINS", str(chains))
    tz, tx, _ = hb.GEOMS[F]
    family = {} if C in (1024, 768) else {"family": "vit"}          # as the two attention budget modules create theirs
    m = native.Model(tz, tx, channels=C, heads=hb.WIDTHS[C].heads, depth=1, head_channels=256, max_batch=max_batch, **family)
    try:
        assert m.channels == C and m.feat_sz == F
        m.load_state_dict(sd)
    except BaseException:
        m.close()
        raise
    return m


def _assert_form(m, form, B):
    """The head bit of the form that runs at B frames is the intended one."""
    from vittracker_amd import native
    bit = m.gemm_form(B) & native.GEMM_HEAD
    assert (bit != 0) == (form == "default"), (form, B, m.gemm_form(B))


def _head(m, X, B):
    """m.head on the frames of X in launches of B -> {map: float64 array}."""
    import torch
    outs = []
    for b0 in range(0, X.shape[0], B):
        out = m.head(torch.from_numpy(np.ascontiguousarray(X[b0:b0 + B])).cuda())
        torch.cuda.synchronize()
        outs.append({k: getattr(out, k).cpu().numpy().astype(np.float64) for k in hb.MAPS})
    return {k: np.concatenate([o[k] for o in outs]) for k in hb.MAPS}


def _check(got, ref, tag, frames=None):
    sl = slice(None) if frames is None else frames
    recs = hb.judge_all({k: got[k][sl] for k in hb.MAPS}, {k: ref["truth"][k][sl] for k in hb.MAPS}, {k: ref["oracle"][k][sl] for k in hb.MAPS})
    for r in recs:
        print(tag, hb.fmt(r))
    assert all(r["finite"] for r in recs), (tag, "not finite")
    assert all(r["ok"] for r in recs), (tag, [hb.fmt(r) for r in recs if not r["ok"]])


def _cases():
    return [pytest.param(C, F, form, name, id=f"{C}-{F}-{form}-{name}") for C in WIDTHS for F in (16, 24) for name in hb.REGIMES
            for form in FORMS if form == "default" or name in ("plain", "one_token")]


@pytest.mark.parametrize("C,F,form,name", _cases())
def test_head_within_budget(C, F, form, name, monkeypatch):
    B = hb.GEOMS[F][2]
    ref = _ref(C, F, name)
    m = _model(C, F, form, ref["sd"], monkeypatch, B)
    try:
        _assert_form(m, form, B)
        got = _head(m, ref["X"], B)
    finally:
        m.close()
    _check(got, ref, f"{C} F={F} {form} {name}")


@pytest.mark.parametrize("C", WIDTHS)
def test_partial_tiles_at_F24(C, monkeypatch):
    ref = _ref(C, 24, "plain", B=1)
    for form in FORMS:
        m = _model(C, 24, form, ref["sd"], monkeypatch, 1)
        try:
            _assert_form(m, form, 1)
            got = _head(m, ref["X"], 1)
        finally:
            m.close()
        _check(got, ref, f"{C} F=24 B=1 {form} plain")


def _clone(out):
    return {k: getattr(out, k).clone() for k in KEYS}


def _passthrough(sd):
    """A copy of `sd` whose block adds exactly nothing to the residual stream (attn.proj and mlp.fc2 zero, weights and biases).  A
    forward and the stage-by-stage chain then hand the SAME f32 rows to the final LayerNorm; with a live block they do not, by design
    and whatever the head does: vb::stem centres block 0's bf16 operand on the position embedding's mean, vb::blocks centres tokens that
    come from outside on each row's own mean (tests/bf16_budget.py), so the block's output differs in its last bf16 roundings."""
    sd = dict(sd)
    for k in ("attn.proj.weight", "attn.proj.bias", "mlp.fc2.weight", "mlp.fc2.bias"):
        sd["backbone.blocks.0." + k] = np.zeros_like(sd["backbone.blocks.0." + k])
    return sd


def test_head_on_a_frame_slice(monkeypatch):
    """A captured step of 3 frames as two chains (VT_GRAPH_CHAINS=2: fork_join over the slices [0, 1) and [1, 3), each with its own frame
    offset into the whole batch's tower-major buffers) against the one-chain step of a second model on the same weights."""
    import torch
    from vittracker_amd import synth
    C, F, B = 768, 24, 3
    sd = _passthrough(hb.state(C, F))          # so that the staged features below are the captured step's own
    tz, tx, _ = hb.GEOMS[F]
    z, x = synth.synth_inputs(31, B, tz, tx)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    one = _model(C, F, "default", sd, monkeypatch, B, chains=1)
    two = _model(C, F, "default", sd, monkeypatch, B, chains=2)
    try:
        whole = _clone(one.forward(zd, xd))
        feat = one.blocks(one.stem(zd, xd))
        torch.cuda.synchronize()
        graph, gout = two.capture(zd, xd)
        graph.launch()
        torch.cuda.synchronize()
        sliced = _clone(gout)
        X = feat.cpu().numpy()
    finally:
        one.close()
        two.close()
    for k in KEYS:
        assert torch.equal(sliced[k], whole[k]), k
    assert not torch.equal(whole["score_map"][0], whole["score_map"][1])
    ref = {"truth": hb.head(sd, X, "truth"), "oracle": hb.head(sd, X, "bf16")}
    got = {k: sliced[k].cpu().numpy().astype(np.float64) for k in hb.MAPS}
    _check(got, ref, "768 F=24 sliced [0,1) + [1,3)")
    for f in range(B):
        _check(got, ref, f"768 F=24 sliced, frame {f}", frames=slice(f, f + 1))


@pytest.mark.parametrize("C", WIDTHS)
def test_forward_head_equals_staged_head(C, monkeypatch):
    import torch
    from vittracker_amd import synth
    F, B = 16, 2
    tz, tx, _ = hb.GEOMS[F]
    z, x = synth.synth_inputs(32, B, tz, tx)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    m = _model(C, F, "default", _passthrough(hb.state(C, F)), monkeypatch, B)
    try:
        whole = _clone(m.forward(zd, xd))
        feat = m.blocks(m.stem(zd, xd))
        torch.cuda.synchronize()
        staged = _clone(m.head(feat))
        torch.cuda.synchronize()
    finally:
        m.close()
    for k in KEYS:
        assert torch.isfinite(whole[k]).all() and torch.equal(staged[k], whole[k]), (C, k)


def test_shrinking_batch_leaves_no_trace(monkeypatch):
    """The zero borders of the maps and the tower slots, which lie elsewhere at B = 1 than at B = 3 ([tower][B frames]), hold nothing of
    the larger batch."""
    import torch
    C, F = 768, 24
    sd = hb.state(C, F)
    big, small = hb.regime("edge_hot", 3, F, C), hb.regime("one_token", 1, F, C)
    res = []
    for warm in (True, False):
        m = _model(C, F, "default", sd, monkeypatch, 3)
        try:
            if warm:
                m.head(torch.from_numpy(big).cuda())
                torch.cuda.synchronize()
            res.append(_clone(m.head(torch.from_numpy(small).cuda())))
            torch.cuda.synchronize()
        finally:
            m.close()
    for k in KEYS:
        assert torch.isfinite(res[0][k]).all() and torch.equal(res[0][k], res[1][k]), k
