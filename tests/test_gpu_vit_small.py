"""GPU: the ViT-Small (width 384, 6 heads) and ViT-Tiny (width 192, 3 heads) OSTrack model points at 128 / 256 and 192 / 384 -- the ViT-Base
kernels at two widths that are no multiple of 256 (vt_create_vit; native.Model(family="vit")), bf16 MFMA against fp32 references.

References: tests/golden/ref_vits_* / ref_vitt_* / ref_vs384_* / ref_vt384_* = outputs of the reference's own VisionTransformer + CenterPredictor
(tests/golden/make_golden_vit_small.py) on the samples `rows` of a seed's 16-sample pool, every one with raw and Hann top-2 margins above 0.03;
the tests run exactly `rows` and excuse no argmax flip.

Tolerances are tests/test_gpu_vitb.py's own, imported: TOL_REL(n) = 2.0e-3 sqrt(n) on the residual stream after n blocks against the rows'
centred norm (the per-block term of that law is relative and has no width in it; K is shorter here), 3.2e-3 on the token stage, TOL_MAP and
TOL_BOX on maps and boxes (depth <= 12, so unscaled).

  1  reference parity      every fixture through native.Model(family="vit") and through build_ostrack (depth 12) / build_small_ostrack
                           (depth 3: the 192 / 384 fixtures are what that builder builds); the stage walk vt_stem -> vt_blocks(nblocks) ->
                           vt_head against the stored activation rows
  2  hazard shapes         both widths, depth 2, synthetic weights: the default route (LayerNorm folded into the GEMMs -- statistics from 6 / 3
                           column slices under a partial 256-wide column tile --, fused qkv + attention at 6 / 3 k-tiles, K = 192 / 1728 on the
                           two-buffer loop) against the plain-LayerNorm unfused route (VB_LN_FOLD=0 VB_FUSED_QKV=0) at B = 1 (320 rows: a partial
                           row tile), B = 3 (960) and, at 192 / 384, B = 1 (720)
  3  narrow == wide        VB_GEMM_NARROW=0 against =1, bit for bit, at B = 1 and 3; vt_gemm_form
  4  exactness             width 192, B = 2, depth 2: template cache, captured graph, uint8 route, one tracking step against its parts, two runs
  5  uint8 / tracking      the ViT-Small uint8 and tracking fixtures
  6  rejections, plugin

Measured on MI355X (this module's printed figures):
  residual stream after 1 / 6 / 12 blocks  1.19e-3 / 2.60e-3 / 3.38e-3 (ViT-Small), 1.18e-3 / 2.66e-3 / 3.50e-3 (ViT-Tiny); depth 3 at 192 / 384 after
                                           1 / 3 blocks: 1.08e-3 / 1.91e-3 and 1.16e-3 / 1.96e-3 (bounds 2.0e-3 / 3.5e-3 / 4.9e-3 / 6.9e-3)
  tokens 2.35e-3 / 2.35e-3 / 2.35e-3 / 2.41e-3 (bound 3.2e-3); uint8 route 1.62e-3 - 1.65e-3
  maps over the six fixtures: score 1.51e-2, size 1.44e-2, offset 3.24e-2; boxes 7.7e-3 (pred and Hann)
  default route against the plain-LayerNorm unfused route, 2 blocks: 1.92e-3 - 2.07e-3 (bound 2.83e-3); maps 1.2e-2 / 8.1e-3 / 3.2e-2
  tracking fixture: every box inside 0.8 of its pixel tolerance, confidence within 4.5e-3

The switches VB_LN_FOLD / VB_FUSED_QKV / VB_GEMM_NARROW are read by vt_create from the environment: a model created while they are set keeps
them, as tests/test_gpu_vitb_narrow.py and tests/test_gpu_vitl.py create theirs, so the routes are compared inside one process; only the
command-line front end runs as a child."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_gpu_vitb import TOL_BOX, TOL_MAP, TOL_REL
from vit_small_cases import ACT_BLOCKS, GEO, PLAIN, TRACK, WIDTHS, cfg_of, load_plain, load_u8, path_of, sd_of, small_cfg
from vitb_u8_fold import MEAN, STD, TOL_TOKENS, rel_c, tokens_truth

pytestmark = pytest.mark.gpu

KEYS = ("score_map", "size_map", "offset_map", "pred_boxes", "hann_boxes", "conf")
_MODELS = {}


def _new_model(model, geo, B, depth, sd, env=None):
    """A family="vit" model created under the environment switches `env` (read at vt_create)."""
    from vittracker_amd import native
    C, heads = WIDTHS[model]
    env = env or {}
    old = {k: os.environ.pop(k, None) for k in ("VB_LN_FOLD", "VB_FUSED_QKV", "VB_GEMM_NARROW")}
    os.environ.update(env)
    try:
        m = native.Model(GEO[geo]["TZ"], GEO[geo]["TX"], channels=C, heads=heads, depth=depth, head_channels=256, max_batch=B, family="vit")
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})
    assert m.channels == C
    m.load_state_dict(sd)
    return m


def _model(model, geo, B, depth, seed, env=None):
    key = (model, geo, B, depth, seed, tuple(sorted((env or {}).items())))
    if key not in _MODELS:
        _MODELS[key] = _new_model(model, geo, B, depth, sd_of(model, geo, depth, seed), env)
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


def _against_fixture(get, g, tag):
    """get(key) -> the tensor of that output"""
    for k, tol in TOL_MAP.items():
        err = float(np.abs(get(k).cpu().numpy() - g[k]).max())
        print(tag, k, err)
        assert err < tol, (k, err)
    eb = float(np.abs(get("pred_boxes").cpu().numpy().reshape(-1, 4) - g["pred_boxes"][:, 0]).max())
    eh = float(np.abs(get("hann_boxes").cpu().numpy() - g["hann_boxes"]).max())
    ec = float(np.abs(get("conf").cpu().numpy() - g["conf"]).max())
    print(tag, "pred_boxes", eb, "hann_boxes", eh, "conf", ec)
    assert eb < TOL_BOX and eh < TOL_BOX and ec < TOL_MAP["score_map"], (eb, eh, ec)


# ------------------------------------------------------------------------------------------------- 1. reference parity
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_forward_matches_the_reference_fixture(name):
    import torch
    model, geo, depth, seed, _, _ = PLAIN[name]
    g, sd, z, x = load_plain(name)
    B, F = int(g["B"]), GEO[geo]["F"]
    m = _model(model, geo, B, depth, seed)
    zd, xd = torch.from_numpy(z).cuda(), torch.from_numpy(x).cuda()
    out = m.forward(zd, xd)
    assert out.score_map.shape == (B, 1, F, F)
    _against_fixture(lambda k: getattr(out, k), g, name)
    bbox, mx = m.cal_bbox(out.score_map, out.size_map, out.offset_map)      # the boxes are the decode of THIS path's own maps
    assert torch.equal(bbox, out.pred_boxes) and torch.equal(mx, out.conf)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_builders_match_the_reference_fixture(name):
    """build_ostrack on the model's YAML (depth 12) or build_small_ostrack (the depth-3 fixtures): load_state_dict, .cuda(), forward."""
    import torch
    from vittracker_amd.model_vitb import build_ostrack, build_small_ostrack
    model, geo, depth, seed, _, _ = PLAIN[name]
    g, sd, z, x = load_plain(name)
    if depth == 3:
        net = build_small_ostrack(small_cfg(model, geo), training=False, max_batch=int(g["B"]))
    else:
        net = build_ostrack(cfg_of(f"{model}_{geo}"), training=False, max_batch=int(g["B"]))
    assert net.depth == depth and net.geom["channels"] == WIDTHS[model][0]
    inc = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not inc.missing_keys and not inc.unexpected_keys
    net = net.cuda().eval()
    out = net.forward(template=torch.from_numpy(z).cuda(), search=torch.from_numpy(x).cuda())
    assert out["pred_boxes"].shape == (int(g["B"]), 1, 4)
    _against_fixture(lambda k: out[k], g, "builder " + name)
    net._native().close()


_ACTS = {}


def _oracle_acts(name):
    """The pinned torch oracle's full activations of the first sample of an activation fixture (tests/test_vit_small_host.py pins the oracle
    to the fixture's stored rows at 2e-4)."""
    import torch
    from oracle import vitb_oracle_torch as ob
    if name not in _ACTS:
        g, sd, z, x = load_plain(name)
        acts = {}
        with torch.no_grad():
            ob.build_from_state(sd, heads=WIDTHS[PLAIN[name][0]][1])(torch.from_numpy(z[:1]), torch.from_numpy(x[:1]), acts)
        _ACTS[name] = acts
    return _ACTS[name]


@pytest.mark.parametrize("name", [n for n in sorted(PLAIN) if PLAIN[n][5]])
def test_each_stage_against_reference_activations(name):
    """The stage calls vt_stem -> vt_blocks(nblocks = k) -> vt_head, held as tests/test_gpu_vitb.py holds them at width 768 (TOL_REL(k) is
    that test's bound on k blocks FED THE ORACLE'S TOKENS): the stem's tokens within 3.2e-3 of the stored rows; blocks[0..k) from the oracle's
    tokens within TOL_REL(k) for every stored k; the final norm from the oracle's last block (f32 arithmetic) within 2e-4; the head from the
    oracle's normalised tokens within TOL_MAP.  (Fed the stem's OWN tokens instead, block 0 of ViT-Small leaves 2.64e-3: the tokens' 2.35e-3
    ride along.  That is the token stage's budget, not a block's, and no bound of the ViT-Base tests covers the sum.)"""
    import torch
    model, geo, depth, seed, _, _ = PLAIN[name]
    g, sd, z, x = load_plain(name)
    LZ, rows = GEO[geo]["LZ"], g["act_rows"]
    acts = _oracle_acts(name)
    m = _model(model, geo, int(g["B"]), depth, seed)
    tok = m.stem(torch.from_numpy(z[:1]).cuda(), torch.from_numpy(x[:1]).cuda())
    e = rel_c(tok[:1, rows].cpu().numpy(), g["act_tokens"])
    print(name, "tokens", e)
    assert e < TOL_TOKENS
    for b in ACT_BLOCKS[depth]:
        _, resid = m.blocks(acts["tokens"].cuda().contiguous(), nblocks=b + 1, want_resid=True)
        e = rel_c(resid[:1, rows].cpu().numpy(), g[f"act_block{b}"])
        print(name, "blocks [0,", b + 1, ")", e, "bound", TOL_REL(b + 1))
        assert e < TOL_REL(b + 1), b
    feat = m.blocks(acts[f"block{depth - 1}"].cuda().contiguous(), nblocks=0)          # final norm only
    srows = [r - LZ for r in rows if r >= LZ]
    np.testing.assert_allclose(feat[:1, srows].cpu().numpy(), g["act_norm"][:, [i for i, r in enumerate(rows) if r >= LZ]], atol=2e-4, rtol=0)
    out = m.head(acts["norm"][:, LZ:].cuda().contiguous())
    for k, tol in TOL_MAP.items():
        err = float(np.abs(getattr(out, k).cpu().numpy() - g[k][:1]).max())
        print(name, "head", k, err)
        assert err < tol, (k, err)


# ------------------------------------------------------------------------------------------------- 2. hazard shapes
PLAIN_ROUTE = {"VB_LN_FOLD": "0", "VB_FUSED_QKV": "0"}


@pytest.mark.parametrize("model,geo,B", [("vits", "256", 1), ("vits", "256", 3), ("vits", "384", 1), ("vitt", "256", 1), ("vitt", "256", 3), ("vitt", "384", 1)])
def test_default_route_agrees_with_the_plain_layernorm_unfused_route(model, geo, B):
    import torch
    C = WIDTHS[model][0]
    m = _model(model, geo, 3 if geo == "256" else 1, 2, 26)
    ref = _model(model, geo, 3 if geo == "256" else 1, 2, 26, PLAIN_ROUTE)
    zd, xd = _inputs(3, B, geo)
    got = {}
    for tag, mm in (("default", m), ("plain", ref)):
        tok = mm.stem(zd, xd)
        feat, resid = mm.blocks(tok.clone(), nblocks=2, want_resid=True)
        out = _clone(mm.forward(zd, xd))
        assert tok.shape == (B, GEO[geo]["LZ"] + GEO[geo]["LX"], C)
        for t in (tok, feat, resid, out.score_map, out.size_map, out.offset_map):
            assert torch.isfinite(t).all(), tag
        got[tag] = (tok.cpu().numpy(), resid.cpu().numpy(), out)
    assert np.array_equal(got["default"][0], got["plain"][0])          # the patch GEMM writes the same f32 rows on either route
    for b in range(B):
        e = rel_c(got["default"][1][b], got["plain"][1][b])
        print(model, geo, B, "frame", b, "residual stream after 2 blocks", e, "bound", TOL_REL(2))
        assert e < TOL_REL(2), (b, e)
    for k, tol in TOL_MAP.items():
        err = float((getattr(got["default"][2], k) - getattr(got["plain"][2], k)).abs().max())
        print(model, geo, B, k, err)
        assert err < tol, (k, err)


# ------------------------------------------------------------------------------------------------- 3. narrow == wide
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64 if t.element_size() == 8 else torch.uint8)


def _run_all(m, model, B):
    """Stem tokens, residual stream, final norm, forward, forward_u8 and one tracking step, every output NaN-filled first."""
    import torch
    from vittracker_amd import native, synth
    C, F, L, LX, nan = WIDTHS[model][0], 16, 320, 256, float("nan")
    zd, xd = _inputs(3, B)
    pd = torch.from_numpy(synth.synth_patches(3, B, 256)).cuda()

    def outputs():
        o = native.Outputs(B, F, "cuda")
        for k in KEYS:
            getattr(o, k).fill_(nan)
        return o
    got = {}
    tok = torch.full((B, L, C), nan, device="cuda")
    native._check(m._L.vt_stem(m._h, native._ptr(zd), native._ptr(xd), B, native._stream(None), native._ptr(tok)), "vt_stem", m._L)
    feat, resid = torch.full((B, LX, C), nan, device="cuda"), torch.full((B, L, C), nan, device="cuda")
    native._check(m._L.vt_blocks(m._h, native._ptr(tok), B, -1, native._stream(None), native._ptr(feat), native._ptr(resid)), "vt_blocks", m._L)
    got["stem"], got["feat"], got["resid"] = tok, feat, resid
    for name, out in (("forward", m.forward(zd, xd, out=outputs())), ("forward_u8", m.forward_u8(zd, pd, out=outputs()))):
        for k in KEYS:
            got[f"{name}.{k}"] = getattr(out, k).clone()
    rs = np.random.RandomState(8)
    frames = torch.from_numpy(rs.randint(0, 256, (2, B, 120, 160, 3)).astype(np.uint8)).cuda()
    states = torch.from_numpy(np.stack([[30 + b, 20 + b, 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)).cuda()
    zc, rf = m.crop(frames[0], states, 2.0, 128, MEAN, STD)
    m.set_template(zc)
    xw, rec, out = torch.empty(B, 3, 256, 256, device="cuda"), torch.full((B, 5), nan, dtype=torch.float64, device="cuda"), outputs()
    m.track_step(frames[1], states, 4.0, MEAN, STD, xw, rf, out, record=rec)
    torch.cuda.synchronize()
    got["step.record"], got["step.states"] = rec.clone(), states.clone()
    for k in KEYS:
        got["step." + k] = getattr(out, k).clone()
    return got


@pytest.mark.parametrize("model,B", [("vits", 1), ("vits", 3), ("vitt", 1), ("vitt", 3)])
def test_narrow_tiles_give_the_wide_tiles_bits(model, B):
    """VB_GEMM_NARROW=0 (ViT-Tiny: the 256 x 256 tile on the two-buffer loop where K = 192, the 256 x 64 tile for conv1's K = 1728) against =1
    (the 128 x 64 ring), fused attention on both: every output array bit for bit."""
    import torch
    wide, narrow = _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "0"}), _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "1"})
    assert wide.gemm_form(B) == 0 and narrow.gemm_form(B) != 0
    a, b = _run_all(wide, model, B), _run_all(narrow, model, B)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.isfinite(a[k].double()).all(), k
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("model", ["vits", "vitt"])
def test_narrow_tiles_give_the_wide_tiles_bits_on_the_unfused_route(model):
    """The same with the q | k projection as a GEMM of its own (VB_FUSED_QKV=0: N = 2 C = 768 / 384, and the v GEMM's transposed store under a
    partial column tile stays on the wide tile in both), at B = 3."""
    import torch
    wide = _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "0", "VB_FUSED_QKV": "0"})
    narrow = _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "1", "VB_FUSED_QKV": "0"})
    zd, xd = _inputs(3, 3)
    outs = []
    for m in (wide, narrow):
        tok = m.stem(zd, xd)
        feat, resid = m.blocks(tok.clone(), nblocks=2, want_resid=True)
        outs.append((tok, feat, resid) + tuple(getattr(_clone(m.forward(zd, xd)), k) for k in KEYS))
    for i, (ta, tb) in enumerate(zip(*outs)):
        assert torch.isfinite(ta.double()).all() and torch.equal(_bits(ta), _bits(tb)), i


def test_gemm_form_reports_what_runs():
    from vittracker_amd import native as N
    every = N.GEMM_PATCH | N.GEMM_PROJ | N.GEMM_FC1 | N.GEMM_FC2 | N.GEMM_HEAD
    for model in ("vits", "vitt"):
        wide, narrow = _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "0"}), _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "1"})
        assert narrow.gemm_form(1) == every and wide.gemm_form(1) == 0          # fused qkv + attention: no q | k GEMM to report
        assert narrow.gemm_form(3) == every and wide.gemm_form(3) == 0
        unfused = _model(model, "256", 3, 2, 26, {"VB_GEMM_NARROW": "1", "VB_FUSED_QKV": "0"})
        assert unfused.gemm_form(1) == every | N.GEMM_QK
        auto = _model(model, "256", 3, 2, 26)
        assert auto.gemm_form(1) == every and auto.gemm_form(256) == 0           # the automatic choice: narrow for one sequence, wide for 256
    g384 = _model("vitt", "384", 1, 2, 26)
    assert g384.gemm_form(1) == every | N.GEMM_QK                                # 192 / 384: always qk GEMM + v GEMM + the streaming kernel


# ------------------------------------------------------------------------------------------------- 4. exactness at width 192
def test_template_cache_graph_and_repeat_are_exact_at_width_192():
    import torch
    from vittracker_amd import synth
    B = 2
    m = _model("vitt", "256", 3, 2, 26)
    zd, xd = _inputs(3, B)
    pd = torch.from_numpy(synth.synth_patches(3, B, 256)).cuda()
    m.set_template(_inputs(4, B)[0])      # another template in the cache: a call with z must not read it
    u_off, f_off = _clone(m.forward_u8(zd, pd)), _clone(m.forward(zd, xd))
    _same(_clone(m.forward(zd, xd)), f_off)                                      # two runs
    _same(_clone(m.forward_u8(zd, pd)), u_off)
    m.set_template(zd)
    _same(_clone(m.forward_u8(None, pd)), u_off)                                 # template cache on == off
    _same(_clone(m.forward(None, xd)), f_off)
    m.set_template_slots(_inputs(5, 1)[0], [1])
    got = _clone(m.forward_u8(None, pd))
    for k in KEYS:
        assert torch.equal(getattr(got, k)[0], getattr(u_off, k)[0]), k
    assert not torch.equal(got.score_map[1], u_off.score_map[1])
    graph, out = m.capture(zd, xd)                                               # captured graph == eager
    for _ in range(2):
        graph.launch()
        torch.cuda.synchronize()
        _same(out, f_off)
    del graph
    assert torch.isfinite(f_off.score_map).all() and not torch.equal(u_off.score_map, f_off.score_map)


def test_forward_u8_against_forward_on_the_normalised_patch_at_width_192():
    """The uint8 route's search tokens within TOL_TOKENS of their fp64 truth (Preprocessor.process, patch embedding, position rows:
    vitb_u8_fold.tokens_truth, the bound tests/test_gpu_patch_u8.py holds ViT-Base to), and its maps within TOL_MAP of vt_forward on the
    normalised patch (two bf16 routes of a depth-2 model, each inside that budget of the fp32 answer)."""
    import torch
    from vittracker_amd import synth
    B, C, LZ = 2, 192, 64
    m = _model("vitt", "256", 3, 2, 26)
    sd = sd_of("vitt", "256", 2, 26)
    zd, _ = _inputs(3, B)
    patches = synth.synth_patches(3, B, 256)
    pd = torch.from_numpy(patches).cuda()
    assert m.patch_u8_supported(B)
    tok = torch.zeros(B, 320, C, device="cuda")
    m.stem_u8(pd, tok)
    truth = tokens_truth(sd, patches)
    for b in range(B):
        e = rel_c(tok[b, LZ:].cpu().numpy(), truth[b])
        print("uint8 tokens, frame", b, e)
        assert e < TOL_TOKENS, (b, e)
    assert not tok[:, :LZ].any()
    u8 = _clone(m.forward_u8(zd, pd))
    f32 = _clone(m.forward(zd, torch.from_numpy(synth.normalise_patches(patches)).cuda()))
    for k, tol in TOL_MAP.items():
        err = float((getattr(u8, k) - getattr(f32, k)).abs().max())
        print("uint8 against fp32 route", k, err)
        assert err < tol, (k, err)


@pytest.mark.parametrize("hw", [(64, 64), (96, 128)])
def test_track_step_equals_the_staged_calls_at_width_192(hw):
    """vt_track_step == vt_crop_u8 + vt_forward_u8(z = None) + vt_update_state_record on two device frames, B = 2, bit for bit."""
    import torch
    from vittracker_amd import native
    H, W = hw
    B, TZ, TX, F = 2, 128, 256, 16
    m = _model("vitt", "256", 3, 2, 26)
    res = {}
    for mode in ("step", "calls"):
        rs = np.random.RandomState(8)
        frames = torch.from_numpy(rs.randint(0, 256, (3, B, H, W, 3)).astype(np.uint8)).cuda()
        states = torch.from_numpy(np.array([[20., 14., 16., 18.], [25., 22., 21., 12.]])).cuda()
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
        res[mode] = recs
    for a, b in zip(res["step"], res["calls"]):
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(ta, tb), i
    assert torch.isfinite(res["step"][-1][0]).all()


def test_two_chain_step_equals_the_one_chain_step_at_width_384(monkeypatch):
    """B = 64 is the smallest batch whose step runs as two chains (VT_GRAPH_CHAINS is read at model creation): it equals the one-chain step
    of a second model on the same weights, bit for bit (depth 1)."""
    import torch
    from vittracker_amd import native
    B, TX, F = 64, 256, 16
    sd = sd_of("vits", "256", 1, 26)
    two = _new_model("vits", "256", B, 1, sd)
    monkeypatch.setenv("VT_GRAPH_CHAINS", "1")
    one = _new_model("vits", "256", B, 1, sd)
    monkeypatch.delenv("VT_GRAPH_CHAINS")
    res = []
    for m in (two, one):
        rs = np.random.RandomState(8)
        frames = torch.from_numpy(rs.randint(0, 256, (2, B, 96, 128, 3)).astype(np.uint8)).cuda()
        states = torch.from_numpy(np.stack([[30 + (b % 40), 20 + (b % 30), 30 + (b % 7), 24 + (b % 5)] for b in range(B)]).astype(np.float64)).cuda()
        z, rf = m.crop(frames[0], states, 2.0, 128, MEAN, STD)
        m.set_template(z)
        x, out, rec = torch.empty(B, 3, TX, TX, device="cuda"), native.Outputs(B, F, "cuda"), torch.zeros(B, 5, dtype=torch.float64, device="cuda")
        m.track_step(frames[1], states, 4.0, MEAN, STD, x, rf, out, record=rec)
        torch.cuda.synchronize()
        res.append([rec.clone(), states.clone()] + [getattr(out, k).clone() for k in KEYS])
        m.close()
    for i, (ta, tb) in enumerate(zip(*res)):
        assert torch.isfinite(ta.double()).all() and torch.equal(ta, tb), i


# ------------------------------------------------------------------------------------------------- 5. uint8 and tracking fixtures (ViT-Small)
def test_forward_u8_matches_the_reference_fixture():
    import torch
    g, sd, z, patches = load_u8()
    B, LZ, L, C = int(g["B"]), 64, 320, 384
    m = _model("vits", "256", 4, 12, int(g["seed"]))
    zd, pd = torch.from_numpy(z).cuda(), torch.from_numpy(patches).cuda()
    out = m.forward_u8(zd, pd)
    _against_fixture(lambda k: getattr(out, k), g, "u8")
    tok = torch.zeros(B, L, C, device="cuda")
    m.stem_u8(pd, tok)
    rows = g["act_rows"]
    sel = [i for i, r in enumerate(rows) if r >= LZ]
    for b in (0, 1):
        e = rel_c(tok[b, rows[sel]].cpu().numpy(), g["act_tokens"][b, sel])
        print("tokens sample", b, e)
        assert e < TOL_TOKENS, (b, e)


def test_tracking_steps_against_the_reference_fixture():
    """tests/test_gpu_vitb_track.py's statement at ViT-Small: one device step per stored frame from the stored state before, the box within
    TOL_BOX * search_size / resize_factor pixels per coordinate, the confidence within TOL_MAP['score_map'].  All 8 frames count."""
    import torch
    from vittracker_amd import host_ops, native, synth
    from vittracker_amd.evaluation.data import synthetic_sequence
    g = dict(np.load(path_of(TRACK), allow_pickle=False))
    seed, n = int(g["seed"]), int(g["n_frames"])
    assert synth.state_checksum(sd_of("vits", "256", 12, seed)) == str(g["state_checksum"])
    m = _model("vits", "256", 1, 12, seed)
    checked = 0
    for q, sseed in enumerate(g["seq_seeds"]):
        seq = synthetic_sequence(f"track_{q}", n + 1, seed=int(sseed))
        z_arr, _, _ = host_ops.sample_target(seq.frames[0], [float(v) for v in seq.ground_truth_rect[0]], 2.0, output_sz=128)
        m.set_template(torch.from_numpy(synth.normalise_patches(z_arr[None], reciprocal=False)).cuda())
        for t in range(1, n + 1):
            states = torch.from_numpy(g["state_before"][q, t - 1][None].copy()).cuda()
            rf, x = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.empty(1, 3, 256, 256, device="cuda")
            out, rec = native.Outputs(1, 16, "cuda"), torch.zeros(1, 5, dtype=torch.float64, device="cuda")
            m.track_step(torch.from_numpy(seq.frames[t][None]).cuda(), states, float(g["search_factor"]), MEAN, STD, x, rf, out, record=rec)
            r = rec.cpu().numpy()[0]
            want_rf = float(g["resize_factor"][q, t - 1])
            assert abs(float(rf[0]) - want_rf) < 1e-12
            tol = TOL_BOX * 256 / want_rf
            err = np.abs(r[:4] - g["box_after"][q, t - 1])
            print(q, t, "box err", err, "tol", tol, "conf err", abs(r[4] - g["conf"][q, t - 1]))
            assert (err <= tol).all(), (q, t, err, tol)
            assert abs(r[4] - g["conf"][q, t - 1]) < TOL_MAP["score_map"], (q, t)
            checked += 1
    assert checked == 8


# ------------------------------------------------------------------------------------------------- 6. rejections and front ends
def test_rejections():
    from vittracker_amd import native, synth
    m = _model("vits", "256", 3, 2, 26)
    with pytest.raises(native.VtError, match=r"candidate elimination is implemented for ViT-Base models \(channels 768\) only"):
        m.set_candidate_elimination([1], [0.7])
    L = native.lib()
    assert L.vt_set_ce_form(m._h, 1) == -1 and b"candidate elimination is implemented for ViT-Base models (channels 768) only" in L.vt_last_error()
    fresh = native.Model(128, 256, channels=384, heads=6, depth=2, head_channels=256, family="vit")
    with pytest.raises(native.VtError) as e:
        fresh.load_state_dict(synth.synth_vitb_state_dict(26, depth=2))          # a 768-wide state dict
    assert "shape mismatch for backbone.patch_embed.proj.weight" in str(e.value) and f"want {384 * 768}" in str(e.value), str(e.value)
    fresh.close()
    # vt_create keeps 384 / 6 / 256 as a shape-generic vit_dist model: it is created, and it wants that family's keys
    generic = native.Model(128, 256, channels=384, heads=6, depth=1, head_channels=256)
    assert generic.channels == 384 and generic.gemm_form(1) == 0
    with pytest.raises(native.VtError, match="missing key"):
        generic.load_state_dict(sd_of("vits", "256", 2, 26))
    generic.close()
    h = ctypes.c_void_p()
    c = native.VtConfig(128, 256, 384, 6, 13, 256, 16, 1)
    assert L.vt_create_vit(ctypes.byref(c), ctypes.byref(h)) == -1 and b"unsupported ViT configuration" in L.vt_last_error()


@pytest.mark.parametrize("name", ["vits_256", "vitt_256"])
def test_tracking_command_line(name, tmp_path):
    """python tracking/test.py ostrack <yaml> --dataset_name synthetic:2x4 --synthetic_weights --batch 2 as a child process: exit 0 and the
    result files of both sequences."""
    import glob
    env = dict(os.environ, VITTRACK_SAVE_DIR=str(tmp_path), VITTRACK_PRJ_DIR=REPO)
    p = subprocess.run([sys.executable, os.path.join(REPO, "tracking", "test.py"), "ostrack", name, "--dataset_name", "synthetic:2x4", "--synthetic_weights",
                        "--batch", "2"], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    boxes = sorted(f for f in glob.glob(os.path.join(str(tmp_path), "**", "*.txt"), recursive=True)
                   if not f.endswith(("_time.txt", "_all_boxes.txt", "_all_scores.txt")))
    assert len(boxes) == 2 and all(name in f for f in boxes), (boxes, p.stdout[-2000:])
    from vittracker_amd.evaluation.data import get_dataset
    frames = {s.name: len(s.frames) for s in get_dataset("synthetic:2x4")}
    assert sorted(os.path.basename(f)[:-4] for f in boxes) == sorted(frames)
    for f in boxes:          # the harness prints and skips a sequence that raises: one finite row per frame says it ran
        rows = [ln for ln in open(f).read().splitlines() if ln.strip()]
        assert len(rows) == frames[os.path.basename(f)[:-4]], (f, rows)
        assert np.isfinite(np.array([[float(v) for v in ln.replace(",", " ").split()] for ln in rows])).all()
