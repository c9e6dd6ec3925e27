"""The bf16 accuracy budget of the ViT MLP chain -- LayerNorm-2 folded into fc1, the fitted GELU of the EPI_GELU epilogue, fc2 onto the residual
stream (vitb.hip, vb_gemm.h, vt_common.h gelu_pair) -- against the fp64 truth, held to a multiple of the error of the oracle that rounds to bf16
where the device does (tests/bf16_budget.py ``run``), per band of the TRUE fc1 pre-activation and per observation.

A plain helper for tests/test_bf16_mlp_budget.py (CPU: the regimes have the stated properties, the observations are exact, the budget has
teeth) and tests/test_gpu_bf16_mlp_budget.py (the device).  It builds on bf16_budget (``bb``): regime, fold, _linear_ln, run, judge, errors, WIDTHS.

Observations: state-dict rewrites after which ``m.blocks(x, nblocks, want_resid=True)`` shows ONE stage (bf16_budget.attn_only's trick).  Every one
zeroes block 0's attn.proj.weight, so attention adds nothing and the residual after proj is x1 = f32(x + proj.bias) exactly; proj.bias is zeroed
as well unless ``keep_bias`` (mean_jump, whose change IS that bias).
  hidden_only(sd, part, w)   depth 1; mlp.fc2.weight = the 0/1 selector of hidden columns [part C, (part + 1) C), fc2.bias = 0: resid - x1 is
                             bf16(GELU(rstd acc + b')) of those columns, exact in the f32 accumulator, up to ONE f32 rounding at |x1 + h| (the
                             floor ``judge(at=)`` and ``judge_bands(at=)`` carry).  Four parts cover the 4 C hidden columns.
  mlp_alone(sd, w)           depth 1; the real fc1 and fc2: resid - x1 is the MLP's f32 update, attention's rounding flips not compounding.
  after_fc2(sd, w)           depth 2; block 0 as in mlp_alone, block 1 = bb.attn_only: resid2 - resid1 is block 1's attention output, computed
                             from the bf16 copy, the slice statistics and the stale mean fc2's epilogue left -- their only consumer.

Truth and oracle: ``bb.run`` on the rewritten state dict, with a hook that records block 0's fc1 pre-activation u, its hidden activations h
and every block's attention output (``stages``; ``reference`` / ``oracle`` cache them).  mode "unfolded" is VB_LN_FOLD=0: the LayerNorm in
full, its output rounded to bf16, W rounded to bf16 without fold or centring.

Regimes (``regime``): functions of (name, L, seed, w) -> (state dict, fp32 tokens); the property of each is asserted in fp64 by
tests/test_bf16_mlp_budget.py at every width and both geometries (``properties``):
  plain          as bb's                                                         none
  gelu_tails     block 0's fc1 weight and bias x FC1_SCALE                       each of the seven bands of the true u holds >= 4 % of the values
  slice_offsets  token columns of 64-column slice s gain a zero-sum offset       between-slice share of every row's variance >= 0.8
                 (+D, -D/2, -D/2 repeating where the slice count is a multiple
                 of 3, +-D alternating otherwise, re-centred), D = SLICE_D
  mean_jump      block 0's proj.weight = 0, proj.bias = +JUMP on every channel   mean^2 / var of x1 - mean(x) >= 25 on every row: the mean the proj
                                                                                 GEMM centres its bf16 copy on (Args::cm) is stale by JUMP
  common_mode    as bb's: the tokens ride on +6, the centring mean is right      none

Judges.  ``judge_bands``: per band of the true pre-activation (edges -6.5, -3, -1, 1, 3, 6.5) the L2 norm of the kernel's error over the band's
elements against FACTORS["band"][band] x the oracle's + the f32 floor; below -6.5 an absolute bound (its docstring).  The hidden slice as a whole,
the MLP update and block 1's attention output go through ``bb.judge`` (rel-L2, max-abs, every (frame, 64-column slice, 16-row tile) slot) under
FACTORS["hidden"], FACTORS["mlp"] and bb.FACTORS["attn"].

Emulated defects (``DEFECTS``, ``emulate``) are applied on top of the oracle; ``CATCHES`` says in which regime and under which judge each must
leave the budget.  fresh_mean_expected is the one that is a defect of the EXPECTATION: the oracle centred on the rows' fresh mean where the
device uses the stale one -- the stale oracle, standing in for the device, must fail it in mean_jump, which shows the budget tells the two apart.
"""
from __future__ import annotations

import numpy as np

import bf16_budget as bb

EDGES = (-6.5, -3.0, -1.0, 1.0, 3.0, 6.5)
BANDS = ("<-6.5", "[-6.5,-3)", "[-3,-1)", "[-1,1)", "[1,3)", "[3,6.5)", ">=6.5")
TAIL_ABS = 1e-9                                    # band "<-6.5": vt_common.h gives the clamp's subtracted term as 2e-10; five times that
REGIMES = ("plain", "gelu_tails", "slice_offsets", "mean_jump", "common_mode")
PARTS = 4

# Amplitudes per width, and the properties they give (fp64, seed 26, B = 2, at 320 / 720 tokens; tests/test_bf16_mlp_budget.py asserts the
# thresholds >= 4 % / >= 0.8 / >= 25).  One row serves every width: u has std 1 before the scale at each, a slice offset is in units of the
# tokens' std 1, and the jump against the rows' std 1.
#   width   FC1_SCALE   smallest band share (gelu_tails)   SLICE_D   smallest between-slice share   JUMP   smallest mean^2 / var (mean_jump)
#   1024    4           5.46 % / 5.36 %                    4         0.934 / 0.934                  6      32.2 / 31.7
#    768    4           5.38 % / 5.40 %                    4         0.873 / 0.868                  6      30.5 / 30.0
#    384    4           5.26 % / 5.44 %                    4         0.855 / 0.855                  6      27.6 / 27.6
#    192    4           5.29 % / 5.36 %                    4         0.838 / 0.838                  6      26.6 / 26.6
# (gelu_tails: u has std 4.02-4.06 and abs-max 19.0-21.9, against std 1.0 and abs-max 4.5-5.5 in every other regime, where the bands past
# |u| = 6.5 are empty and those past 3 hold 0.1-0.2 % each.  The +-D pattern of the 16 slices of width 1024 puts D^2 between the slices, the
# three-slice pattern D^2 / 2: hence the larger share there.)
AMPS = {c: {"FC1_SCALE": 4.0, "SLICE_D": 4.0, "JUMP": 6.0} for c in bb.WIDTHS}

# error(kernel) / error(bf16 oracle) allowed.  "band": per band of the true pre-activation (hidden_only, judge_bands); "hidden": the hidden
# slice as a whole; "mlp": the MLP's f32 update (mlp_alone) -- the last two for rel-L2, max-abs and the worst (frame, 64-column slice, 16-row
# tile) slot, as bb.FACTORS.  after_fc2 runs under bb.FACTORS["attn"].  Set from ONE MI355X run of tests/test_gpu_bf16_mlp_budget.py's cases,
# each against the oracle (never the kernel's own output), as 1.5 x the worst ratio seen over forms, widths and regimes; the cap, a third of
# the smallest ratio a defect reaches under the judge in its catching regime, is asserted by tests/test_bf16_mlp_budget.py (x1.70 bands,
# x2.02 hidden, x1.55 mlp).  Measured, 153 cases / 282 judged rows, the narrow and the wide form alike to every printed digit:
#   bands    [-6.5,-3) x1.00, x1.01 in common_mode at 768; every other band x1.00 at every width, form and regime; below -6.5 (gelu_tails
#            only, 5.2-5.5 % of a part) |resid - x1| <= 4.7e-10 = one f32 ulp of the smallest |x1| there, bounds 2.3e-7 .. 2.6e-7
#   hidden   rel-L2 x1.00 / max-abs x1.00 / worst slot x1.00-1.02 (1024, 384: <= x1.01)          [kernel - oracle 0.00-0.03 of the oracle's
#            error, common_mode 0.03-0.07]
#   mlp      x1.00 / x1.00 / x1.00-1.01, partial tiles and each frame on its own x1.00; VB_LN_FOLD=0 against the unfolded oracle x1.00 /
#            x1.00 / x1.00-1.01                                                                   [0.00-0.02, unfolded 0.02-0.05]
#   attn     (after_fc2, fused = unfused) x1.00 / x1.00 / x1.01-1.02, plain at 768 slot x1.17     [0.09-0.31]
# mean_jump is x1.00 like the rest: the device pays the stale mean exactly as the oracle says (hidden 1.41e-2 .. 1.49e-2 per part, the
# update 1.42e-2 folded against 3.33e-3 with VB_LN_FOLD=0: x4.26, the oracle's own ratio).
FACTORS = {"band": {b: 1.52 if b == BANDS[1] else 1.5 for b in BANDS[1:]}, "hidden": 1.53, "mlp": 1.52}

# which (regime, judge) must fail each emulated defect; judges: "bands" (judge_bands on a hidden part), "hidden", "mlp", "attn" (after_fc2)
CATCHES = {
    "gelu_tail_dropped": (("plain", "bands"), ("gelu_tails", "bands")),
    "gelu_tanh": (("plain", "bands"), ("gelu_tails", "bands")),
    "gelu_clamp3": (("plain", "bands"), ("gelu_tails", "bands")),
    "gelu_no_clamp": (("gelu_tails", "bands"), ("gelu_tails", "hidden"), ("gelu_tails", "mlp")),
    "relu_below_m1": (("plain", "bands"), ("gelu_tails", "bands")),
    "merge_no_between": (("slice_offsets", "bands"), ("slice_offsets", "hidden"), ("slice_offsets", "mlp"), ("slice_offsets", "attn")),
    "rstd_row16": (("plain", "hidden"), ("plain", "mlp")),
    "no_W_beta": (("plain", "hidden"), ("plain", "mlp")),
    "fresh_mean_expected": (("mean_jump", "hidden"), ("mean_jump", "mlp")),
    "fc2_drop_last_ktile": (("plain", "mlp"),),
    "fc2_swap_kstep": (("plain", "mlp"),),
    "hidden_part_shift": (("plain", "bands"), ("plain", "hidden")),
}
DEFECTS = tuple(CATCHES)

# vt_common.h gelu_pair: P(-t), the degree-6 fit of log2 erfc(t / sqrt 2), highest power first (in nt = -t), and its clamp
GELU_COEF = (2.992413958e-05, 7.398738213e-04, 7.977461502e-03, 5.323818492e-02, -4.589156874e-01, 1.151147082e+00, -1.0)
GELU_CLAMP = 6.5


# ----------------------------------------------------------------------------- GELU forms
def gelu(u):
    return 0.5 * u * (1.0 + bb._erf(u / np.sqrt(2.0)))


def gelu_fit(u, clamp=GELU_CLAMP):
    """gelu_pair transcribed, evaluated in f32 (numpy rounds every step where the device fuses multiply and add); clamp None: without it."""
    u = np.asarray(u, np.float32)
    nt = -np.abs(u)
    if clamp is not None:
        nt = np.maximum(nt, np.float32(-clamp))
    with np.errstate(over="ignore", invalid="ignore"):
        p = nt * np.float32(GELU_COEF[0]) + np.float32(GELU_COEF[1])
        for c in GELU_COEF[2:]:
            p = p * nt + np.float32(c)
        return (nt * np.exp2(p) + np.maximum(u, np.float32(0))).astype(np.float64)


def _gelu_defect(defect, u):
    t = np.abs(u)
    if defect == "gelu_tail_dropped":                  # the subtracted term t * 0.5 erfc(t / sqrt 2) dropped past |u| = 3
        return np.where(t > 3.0, np.maximum(u, 0.0), gelu(u))
    if defect == "gelu_tanh":
        return 0.5 * u * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))
    if defect == "gelu_clamp3":                        # t clamped at 3 where gelu_pair clamps at 6.5
        tc = np.minimum(t, 3.0)
        return np.maximum(u, 0.0) - tc * 0.5 * (1.0 - bb._erf(tc / np.sqrt(2.0)))
    if defect == "gelu_no_clamp":
        return gelu_fit(u, clamp=None)
    if defect == "gelu_fit":                           # no defect: the device's own form (tests/test_bf16_mlp_budget.py holds it inside every band)
        return gelu_fit(u)
    if defect == "relu_below_m1":
        return np.where(u < -1.0, 0.0, gelu(u))
    raise KeyError(defect)


# ----------------------------------------------------------------------------- regimes
def _slice_offsets(C, D):
    P = C // bb.HD
    pat = (D, -D / 2, -D / 2) if P % 3 == 0 else (D, -D)
    off = np.array([pat[s % len(pat)] for s in range(P)], np.float64)
    return np.repeat(off - off.mean(), bb.HD)


def regime(name, L, seed=26, B=2, depth=1, w=bb.W768):
    """(state dict, fp32 tokens (B, L, C)) of MLP regime `name` at L = 320 or 720 tokens and width w, at that width's amplitudes (AMPS)."""
    assert name in REGIMES, name
    amp = AMPS[w.C]
    sd, X = bb.regime("common_mode" if name == "common_mode" else "plain", L, seed, B, depth, w)
    p = "backbone.blocks.0."
    if name == "gelu_tails":
        for k in ("mlp.fc1.weight", "mlp.fc1.bias"):
            sd[p + k] = (sd[p + k].astype(np.float64) * amp["FC1_SCALE"]).astype(np.float32)
    if name == "slice_offsets":
        X = (X.astype(np.float64) + _slice_offsets(w.C, amp["SLICE_D"])).astype(np.float32)
    if name == "mean_jump":
        sd[p + "attn.proj.weight"] = np.zeros_like(sd[p + "attn.proj.weight"])
        sd[p + "attn.proj.bias"] = np.full(w.C, amp["JUMP"], np.float32)
    return sd, X


def keeps_bias(name):
    return name == "mean_jump"


# ----------------------------------------------------------------------------- observations
def _proj_off(sd, keep_bias, w):
    sd = dict(sd)
    p = "backbone.blocks.0.attn.proj."
    sd[p + "weight"] = np.zeros((w.C, w.C), np.float32)
    if not keep_bias:
        sd[p + "bias"] = np.zeros(w.C, np.float32)
    return sd


def hidden_only(sd, part, w=bb.W768, keep_bias=False):
    """A depth-1 copy of `sd` whose block returns x1 + bf16(GELU(fc1(LN(x1))))[:, part C : (part + 1) C]."""
    assert 0 <= part < PARTS
    sd = _proj_off(sd, keep_bias, w)
    C = w.C
    sel = np.zeros((C, PARTS * C), np.float32)
    sel[np.arange(C), part * C + np.arange(C)] = 1.0
    sd["backbone.blocks.0.mlp.fc2.weight"] = sel
    sd["backbone.blocks.0.mlp.fc2.bias"] = np.zeros(C, np.float32)
    return sd


def mlp_alone(sd, w=bb.W768, keep_bias=False):
    """A copy of `sd` whose block 0 returns x1 + MLP(x1), x1 = x + proj.bias (0 unless keep_bias)."""
    return _proj_off(sd, keep_bias, w)


def after_fc2(sd, w=bb.W768, keep_bias=False):
    """A depth-2 copy of `sd`: block 0 as in mlp_alone, block 1 returns x + attention(x)."""
    return bb.attn_only(mlp_alone(sd, w, keep_bias), 1, w)


# ----------------------------------------------------------------------------- truth and oracle
def rstd_no_between(x):
    """The rstd a merge of the 64-column slice statistics gives when it forgets the between-slice term 64 (mean_s - mean)^2."""
    s = x.reshape(*x.shape[:-1], -1, bb.HD)
    return 1.0 / np.sqrt(s.var(-1).mean(-1) + bb.LN_EPS)


def _defect_sd(sd, defect, w):
    if defect not in ("fc2_drop_last_ktile", "fc2_swap_kstep"):
        return sd
    sd = dict(sd)
    k = "backbone.blocks.0.mlp.fc2.weight"
    W = np.array(sd[k])
    if defect == "fc2_drop_last_ktile":                # hidden columns 4 C - 64 .. 4 C - 1 never multiplied
        W[:, -bb.KC:] = 0.0
    else:                                              # the two 32-deep halves of k-tile 0 exchanged on ONE operand
        W[:, :64] = W[:, np.r_[32:64, 0:32]]
    sd[k] = W
    return sd


def stages(sd, X, w=bb.W768, nblocks=1, mode="truth", defect=None, fresh=False, chunk=None):
    """bb.run on `sd` with the per-stage hook: {"res": residual after each block, "x1" / "u" / "h" / "ao": per block the residual after proj,
    the fc1 pre-activation, the hidden activations, the attention output, "upd": block 0's MLP update h W2^T + b2 before it meets x1}.
    defect: one of DEFECTS emulated on top of the oracle (mode "bf16")."""
    assert defect is None or mode == "bf16"
    rec = {k: [None] * nblocks for k in ("x1", "u", "h", "ao")}
    p = "backbone.blocks.0."
    at_stats = (nblocks - 1, "rstd1") if nblocks == 2 else (0, "rstd2")        # after_fc2: the statistics fc2 left, read by block 1's qkv

    def hook(i, stage, v):
        if stage in ("rstd1", "rstd2"):
            if (i, stage) != at_stats:
                return None
            if defect == "merge_no_between":
                return rstd_no_between(v)
            if defect == "rstd_row16":                 # the epilogue reads the rstd of row m + 16
                return np.roll(bb._stats(v)[2], -16, axis=1)
            return None
        out = None
        if i == 0 and stage == "u" and defect == "no_W_beta":
            out = v - bb.f32(bb._w(sd, p + "mlp.fc1.weight") @ bb._w(sd, p + "norm2.bias"))
        if i == 0 and stage == "h" and defect is not None and defect.startswith(("gelu_", "relu_")):
            out = bb.bf16(_gelu_defect(defect, rec["u"][0]))
        if stage in rec:
            rec[stage][i] = v if out is None else out
        return out

    run_sd = _defect_sd(sd, defect, w)
    with np.errstate(over="ignore", invalid="ignore"):
        res, _ = bb.run(run_sd, X, nblocks, mode, chunk=chunk, w=w, hook=hook, fresh=fresh)
        W2 = bb._w(run_sd, p + "mlp.fc2.weight")
        rec["upd"] = rec["h"][0] @ (W2 if mode == "truth" else bb.bf16(W2)).T + bb._w(run_sd, p + "mlp.fc2.bias")
    rec["res"] = res
    return rec


def reference(name, L, w=bb.W768, B=2, seed=26, depth=1):
    """The CPU reference of regime `name`: the state dict of the mlp_alone (depth 1) or after_fc2 (depth 2) model, the tokens, the truth's
    stages; ``oracle`` adds the oracle's per (mode, defect, fresh, chunk)."""
    raw, X = regime(name, L, seed, B, depth, w)
    keep = keeps_bias(name)
    sd = mlp_alone(raw, w, keep) if depth == 1 else after_fc2(raw, w, keep)
    return {"name": name, "L": L, "w": w, "B": B, "depth": depth, "keep": keep, "sd": sd, "X": X, "truth": stages(sd, X, w, depth), "oracle": {}}


def oracle(ref, mode="bf16", defect=None, fresh=False, chunk=None):
    key = (mode, defect, fresh, chunk)
    if key not in ref["oracle"]:
        ref["oracle"][key] = stages(ref["sd"], ref["X"], ref["w"], ref["depth"], mode, defect, fresh, chunk)
    return ref["oracle"][key]


def part_of(a, part, w):
    return a[..., part * w.C:(part + 1) * w.C]


def view(S, judge, w, part=0):
    """What judge "bands" / "hidden" (hidden columns of `part`), "mlp" (the update) or "attn" (block 1's attention output) compares, of stages S."""
    if judge in ("bands", "hidden"):
        return part_of(S["h"][0], part, w)
    return S["upd"] if judge == "mlp" else S["ao"][1]


def emulate(ref, defect, judge, part=0):
    """(kernel stand-in, expected oracle) of `defect` under `judge`: the defective oracle against the oracle -- but for fresh_mean_expected,
    where the oracle as it is stands in for the device and the EXPECTED oracle is the one centred on the fresh mean."""
    w = ref["w"]
    if defect == "fresh_mean_expected":
        return view(oracle(ref), judge, w, part), view(oracle(ref, fresh=True), judge, w, part)
    if defect == "hidden_part_shift":
        return view(oracle(ref), judge, w, (part + 1) % PARTS), view(oracle(ref), judge, w, part)
    return view(oracle(ref, defect=defect), judge, w, part), view(oracle(ref), judge, w, part)


# ----------------------------------------------------------------------------- regime properties (fp64)
def band_index(u):
    """0 .. 6: the band of BANDS each pre-activation lies in; band k >= 1 is [EDGES[k - 1], EDGES[k])."""
    return np.searchsorted(np.asarray(EDGES), u, side="right")


def properties(name, L, w=bb.W768, B=2, seed=26):
    """What tests/test_bf16_mlp_budget.py asserts of regime `name`, in fp64: x1 = x + proj.bias as every observation has it, and the true
    fc1 pre-activation of block 0 (what stages(...)["x1"][0] / ["u"][0] of the truth hold; attention is not run for it)."""
    sd, X = regime(name, L, seed, B, 1, w)
    sd = mlp_alone(sd, w, keeps_bias(name))
    x = np.asarray(X, np.float64)
    x1 = x + bb._w(sd, "backbone.blocks.0.attn.proj.bias")
    u = bb._linear_ln(sd, "backbone.blocks.0.", "norm2", "mlp.fc1", x1, "truth", None)
    share = np.bincount(band_index(u).ravel(), minlength=len(BANDS)) / u.size
    mean, xc, _ = bb._stats(x1)
    sm = x1.reshape(*x1.shape[:-1], -1, bb.HD).mean(-1) - mean[..., None]
    op = x1 - x.mean(-1, keepdims=True)                 # what the proj GEMM rounds to bf16
    return {"band_share": share, "band_share_min": float(share.min()), "u_std": float(u.std()), "u_absmax": float(np.abs(u).max()),
            "between_share_min": float(((sm * sm).mean(-1) / (xc * xc).mean(-1)).min()),
            "mean2_var_min": float((op.mean(-1) ** 2 / op.var(-1)).min())}


# ----------------------------------------------------------------------------- the budget
def judge_bands(got, truth_h, oracle_h, u_truth, at, factors=None):
    """The hidden activations per band of the TRUE pre-activation u_truth (all arrays the same shape): per band the L2 norm of the kernel's
    error over the band's elements, the oracle's likewise, the floor FLOOR_ULPS ulps of f32 at `at` (the values the observed quantity was
    rounded at), ok = err_k <= F_band * err_o + floor.  An empty band passes.  Below -6.5 the oracle's error is ~3e-12 and no ratio means
    anything: there the bound is absolute, |got| <= floor + TAIL_ABS per element -- with the observation resid - x1 that resolves the band
    only to the f32 rounding at |x1|: it says that the clamp leaves nothing visible there, not what the 2e-10 term is.
    factors: one number for every band, or a dict per band; default FACTORS["band"]."""
    f = FACTORS["band"] if factors is None else factors
    got, truth_h, oracle_h, u_truth, at = (np.asarray(a, np.float64) for a in (got, truth_h, oracle_h, u_truth, at))
    assert got.shape == truth_h.shape == oracle_h.shape == u_truth.shape == at.shape
    idx = band_index(u_truth)
    rows, ok = [], True
    finite = bool(np.isfinite(got).all())
    for b, name in enumerate(BANDS):
        mk = idx == b
        n = int(mk.sum())
        row = {"band": name, "n": n, "share": n / idx.size, "kernel": 0.0, "oracle": 0.0, "floor": 0.0, "ratio": float("nan"), "ok": True}
        if n:
            g, fl = got[mk], bb.FLOOR_ULPS * bb.EPS32 * np.abs(at[mk])
            with np.errstate(invalid="ignore"):
                if b == 0:
                    row.update(kernel=float(np.abs(g).max()) if np.isfinite(g).all() else float("inf"), oracle=float(np.abs(oracle_h[mk] - truth_h[mk]).max()),
                               floor=float(fl.max()) + TAIL_ABS)
                    row["ok"] = bool((np.abs(g) <= fl + TAIL_ABS).all())
                else:
                    ek, eo = float(np.linalg.norm(g - truth_h[mk])), float(np.linalg.norm(oracle_h[mk] - truth_h[mk]))
                    fb = f[name] if isinstance(f, dict) else f
                    row.update(kernel=ek, oracle=eo, floor=float(np.linalg.norm(fl)), ratio=ek / max(eo, 1e-300), factor=fb)
                    row["ok"] = bool(np.isfinite(ek) and ek <= fb * eo + row["floor"])
        ok = ok and row["ok"]
        rows.append(row)
    ratios = [r["ratio"] for r in rows[1:] if r["n"]]
    return {"bands": rows, "finite": finite, "ok": ok and finite, "worst_ratio": float(np.nanmax(ratios)) if ratios else float("nan")}


def fmt_bands(r):
    cells = []
    for row in r["bands"]:
        if not row["n"]:
            cells.append(f"{row['band']} -")
        elif row["band"] == BANDS[0]:
            cells.append(f"{row['band']} {row['share']:.1%} |got| {row['kernel']:.1e} (bound {row['floor']:.1e})" + ("" if row["ok"] else " OVER"))
        else:
            cells.append(f"{row['band']} {row['share']:.1%} {row['kernel']:.2e} x{row['ratio']:.2f}" + ("" if row["ok"] else " OVER"))
    return "  bands: " + " | ".join(cells)


def judge_stage(stage, got, truth, oracle_, at, w, factor=None):
    """bb.judge on one observation under this module's factor ("hidden", "mlp") or bb's ("attn"); slots are (frame, 64-column slice, 16-row tile)."""
    f = factor if factor is not None else (bb.FACTORS["attn"] if stage == "attn" else FACTORS[stage])
    return bb.judge(stage, got, truth, oracle_, factor=f, at=at, w=w)


def reach(r):
    """The largest error ratio against the oracle a judged row shows: what a factor has to stay a third of for an emulated defect."""
    if "bands" in r:
        return r["worst_ratio"] if r["finite"] else float("inf")
    return max(r["ratio_rel"], r["ratio_abs"], r["slot_ratio"]) if r["finite"] else float("inf")
