"""GPU: the ViT MLP chain -- LayerNorm-2 folded into fc1, the fitted GELU of the EPI_GELU epilogue, fc2 onto the residual stream, and the bf16
copy / slice statistics / stale mean fc2's epilogue leaves -- against the fp64 truth, held to a multiple of the bf16 oracle's own error on
the same input (tests/bf16_mlp_budget.py), per band of the true fc1 pre-activation and per observation:

  test_hidden_bands    hidden_only: resid - x1 is bf16(GELU(rstd acc + b')) of one quarter of the hidden columns.  Widths 768 and 192 (the
                       A_ANYK two-buffer loop; N = 768 / 192 under padded 256-wide tiles) at 320 tokens, B = 2, all five regimes, all four
                       parts, on the narrow 128 x 64 tile (VB_GEMM_NARROW=1) and the wide 256 x 256 one (=0); widths 1024 and 384 run plain,
                       gelu_tails and slice_offsets on the default form.  judge_bands + the hidden slice as a whole.
  test_mlp_alone       the same widths and forms, regimes plain, gelu_tails, slice_offsets, mean_jump: resid - x1 is the MLP's f32 update.
  test_after_fc2       widths 768 and 192, regimes plain, slice_offsets, mean_jump: block 1's attention output, computed from what fc2's
                       epilogue left, on the fused route and with VB_FUSED_QKV=0, where the qk GEMM reads rstd.  bb.FACTORS["attn"].
  test_partial_tiles   plain and gelu_tails at 768 with a partial last tile: B = 1 at 320 tokens (256 + 64 rows), B = 1 at 720 (512 + 208),
                       B = 3 at 320 (3.75 tiles); wide and narrow; test_mlp_alone's judge, each frame on its own as well.
  test_unfolded        VB_LN_FOLD=0 at 768, regimes plain, slice_offsets, mean_jump, against the ``unfolded`` oracle; mean_jump prints the
                       folded / unfolded error ratio, the measured cost of the stale centring mean.

One model per case, built at max_batch = B, the switches read at model creation set and cleared with monkeypatch.  The CPU references are
built once per (width, tokens, regime, B, depth) in the module's order of cases; a case is one or two launches.  Asserted: finite everywhere,
err(kernel) <= factor x err(oracle) + floor per band (below -6.5: |got| <= floor + 1e-9), and for rel-L2, max-abs and every (frame,
64-column slice, 16-row tile) slot of the other observations.  Every case prints its fmt rows.  The kernel - oracle distance is printed,
not asserted: behind the GELU it is not stably below half of the oracle's error (bf16_budget.KO_FRAC's comment).

Measured on one MI355X run: bf16_mlp_budget.FACTORS' comment and NOTES.md."""
import numpy as np
import pytest

import bf16_budget as bb
import bf16_mlp_budget as mb

pytestmark = pytest.mark.gpu

FORMS = {"default": None, "narrow": "1", "wide": "0"}          # VB_GEMM_NARROW at model creation
SWITCHES = ("VB_GEMM_NARROW", "VB_GEMM_NARROW_FILL", "VB_FUSED_QKV", "VB_ATTN_STREAM", "VB_LN_FOLD", "VB_LN_CENTER")
FULL_WIDTHS, DEFAULT_WIDTHS = (768, 192), (1024, 384)          # every form and regime | the default form, three regimes
DEFAULT_REGIMES = ("plain", "gelu_tails", "slice_offsets")
ALONE_REGIMES = ("plain", "gelu_tails", "slice_offsets", "mean_jump")
FC2_REGIMES = ("plain", "slice_offsets", "mean_jump")
_REF = {}


def _ref(C, L, name, B=2, depth=1):
    """The CPU reference of a (width, tokens, regime, B, depth), kept while the module's cases stay on it (the last two are held)."""
    key = (C, L, name, B, depth)
    if key not in _REF:
        while len(_REF) >= 2:
            _REF.pop(next(iter(_REF)))
        _REF[key] = mb.reference(name, L, bb.WIDTHS[C], B=B, depth=depth)
    return _REF[key]


def _resid(C, L, B, depth, sd, X, env, monkeypatch, nblocks=(1,)):
    """The f32 residual after each of `nblocks` blocks, as float64, of a model created under `env` on state dict sd."""
    import torch
    from vittracker_amd import native
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)
    tz, tx = bb.SIZES[L]
    family = {} if C >= 768 else {"family": "vit"}          # as the sibling budget modules create theirs
    m = native.Model(tz, tx, channels=C, heads=bb.WIDTHS[C].heads, depth=depth, head_channels=256, max_batch=B, **family)
    try:
        assert m.channels == C and m.L == L
        m.load_state_dict(sd)
        x = torch.from_numpy(X).cuda()
        out = [m.blocks(x, nblocks=k, want_resid=True)[1].cpu().numpy().astype(np.float64) for k in nblocks]
    finally:
        m.close()
    for r in out:
        assert r.shape == (B, L, C) and np.isfinite(r).all()
    return out


def _check(r, tag):
    print(tag, bb.fmt(r))
    assert r["finite"], (tag, "not finite")
    assert r["ok"], (tag, bb.fmt(r))


def _cases(full_regimes, parts=(None,)):
    out = []
    for C in FULL_WIDTHS + DEFAULT_WIDTHS:
        for name in (full_regimes if C in FULL_WIDTHS else DEFAULT_REGIMES):
            for form in (("narrow", "wide") if C in FULL_WIDTHS else ("default",)):
                for part in parts:
                    ps = (C, form, name) + (() if part is None else (part,))
                    out.append(pytest.param(*ps, id="-".join(str(p) for p in ps)))
    return out


@pytest.mark.parametrize("C,form,name,part", _cases(mb.REGIMES, range(mb.PARTS)))
def test_hidden_bands(C, form, name, part, monkeypatch):
    w, L, B = bb.WIDTHS[C], 320, 2
    ref = _ref(C, L, name)
    T, O = ref["truth"], mb.oracle(ref)
    sd = mb.hidden_only(ref["sd"], part, w, keep_bias=True)          # (the reference's state dict already carries the regime's proj.bias)
    resid, = _resid(C, L, B, 1, sd, ref["X"], {"VB_GEMM_NARROW": FORMS[form]}, monkeypatch)
    x1 = O["x1"][0]
    got, truth, orc, u = resid - x1, mb.part_of(T["h"][0], part, w), mb.part_of(O["h"][0], part, w), mb.part_of(T["u"][0], part, w)
    tag = f"{C} {form} {name} part {part}"
    rb = mb.judge_bands(got, truth, orc, u, x1 + truth)
    rh = mb.judge_stage("hidden", got, truth, orc, x1 + truth, w)
    print(tag, bb.fmt(rh))
    print(tag, mb.fmt_bands(rb))
    assert rh["finite"] and rb["finite"], (tag, "not finite")
    assert rh["ok"], (tag, bb.fmt(rh))
    assert rb["ok"], (tag, mb.fmt_bands(rb))


def _mlp_rows(ref, O, resid, tag, frames=False):
    w, T = ref["w"], ref["truth"]
    x1 = O["x1"][0]
    got, truth, orc = resid - x1, T["upd"], O["upd"]
    at = x1 + truth
    rows = [mb.judge_stage("mlp", got, truth, orc, at, w)]
    _check(rows[0], tag)
    if frames:
        for f in range(ref["B"]):
            rows.append(mb.judge_stage("mlp", got[f:f + 1], truth[f:f + 1], orc[f:f + 1], at[f:f + 1], w))
            _check(rows[-1], f"{tag} frame {f}")
    return rows


@pytest.mark.parametrize("C,form,name", _cases(ALONE_REGIMES))
def test_mlp_alone(C, form, name, monkeypatch):
    ref = _ref(C, 320, name)
    resid, = _resid(C, 320, 2, 1, ref["sd"], ref["X"], {"VB_GEMM_NARROW": FORMS[form]}, monkeypatch)
    _mlp_rows(ref, mb.oracle(ref), resid, f"{C} {form} {name}")


@pytest.mark.parametrize("route", ["fused", "unfused"])
@pytest.mark.parametrize("name", FC2_REGIMES)
@pytest.mark.parametrize("C", FULL_WIDTHS)
def test_after_fc2(C, name, route, monkeypatch):
    w, L, B = bb.WIDTHS[C], 320, 2
    ref = _ref(C, L, name, depth=2)
    T, O = ref["truth"], mb.oracle(ref)
    r1, r2 = _resid(C, L, B, 2, ref["sd"], ref["X"], {"VB_FUSED_QKV": "0" if route == "unfused" else None}, monkeypatch, nblocks=(1, 2))
    _check(mb.judge_stage("attn", r2 - r1, T["ao"][1], O["ao"][1], T["res"][0] + T["ao"][1], w), f"{C} {route} {name}")


@pytest.mark.parametrize("form", ["wide", "narrow"])
@pytest.mark.parametrize("B,L", [(1, 320), (1, 720), (3, 320)])
@pytest.mark.parametrize("name", ["plain", "gelu_tails"])
def test_partial_tiles(name, B, L, form, monkeypatch):
    ref = _ref(768, L, name, B=B)
    resid, = _resid(768, L, B, 1, ref["sd"], ref["X"], {"VB_GEMM_NARROW": FORMS[form]}, monkeypatch)
    _mlp_rows(ref, mb.oracle(ref), resid, f"768 {form} {name} B {B} L {L}", frames=True)


@pytest.mark.parametrize("name", FC2_REGIMES)
def test_unfolded(name, monkeypatch):
    ref = _ref(768, 320, name)
    resid, = _resid(768, 320, 2, 1, ref["sd"], ref["X"], {"VB_LN_FOLD": "0"}, monkeypatch)
    unf, = _mlp_rows(ref, mb.oracle(ref, mode="unfolded"), resid, f"768 unfolded {name}")
    if name == "mean_jump":          # the same model folded: the stale centring mean's cost on the device, next to the oracles'
        resid, = _resid(768, 320, 2, 1, ref["sd"], ref["X"], {}, monkeypatch)
        fol, = _mlp_rows(ref, mb.oracle(ref), resid, f"768 folded {name}")
        print(f"768 mean_jump folded / unfolded rel-L2 of the MLP update: device {fol['kernel_rel']:.2e} / {unf['kernel_rel']:.2e} = "
              f"x{fol['kernel_rel'] / unf['kernel_rel']:.2f}, oracle {fol['oracle_rel']:.2e} / {unf['oracle_rel']:.2e} = x{fol['oracle_rel'] / unf['oracle_rel']:.2f}")
