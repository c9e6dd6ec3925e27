"""The bf16 accuracy budget of the ViT-Base attention routes: a kernel's error against the fp64 truth, held to a multiple of the error
of an oracle that rounds to bf16 where the device does, on the same input -- per softmax regime.

A plain helper for tests/test_bf16_budget.py (CPU: the regimes have the stated properties, the budget has teeth) and
tests/test_gpu_bf16_budget.py (the four routes on the device), modelled on tests/fp32_budget.py.

Observing attention alone.  A depth-1 model whose attn.proj.weight is the identity (exact in bf16; ao x I is exact in the f32
accumulator), whose proj.bias is 0 and whose mlp.fc2 weight and bias are 0 (``attn_only``) returns from
``m.blocks(x, nblocks=1, want_resid=True)`` the f32 value x + ao: ``resid - x`` in fp64 is the attention kernel's bf16 output for
every frame, row and head, up to ONE f32 rounding at |x + ao| <= FLOOR_ULPS ulps of it.  ``judge`` adds that floor to the bound
(``at`` = the array the rounding happens at), as fp32_budget.judge does.

Truth and oracle (``run``).  Truth: the block in fp64 from the fp32 tokens.  Oracle ("bf16"): the same block with
  * the LayerNorm folded into qkv / fc1 as vitb.hip fold_layernorm does (W' = W g - mean_k(W g), b' = b + W beta, in fp64, W' through
    f32 to bf16, the q rows times 2^-3) and the operand the CENTRED raw row bf16(x - c) (vb_gemm.h Args::cm): c = the row's own mean
    for tokens from outside (vbm::layernorm_kernel), the mean the row had BEFORE the last update for a row a GEMM just wrote;
  * q, k, v rounded to bf16 after rstd * acc + b';
  * P rounded to bf16 for P.V, the row sum from the unrounded P, exp against the row maximum (``chunk=None``: vba::attn_kernel and
    vbq::qkv_attn_kernel) or against the running maximum of 64-key chunks with l and O rescaled (``chunk=64``: vbs::attn_stream_kernel);
  * the attention output, the GELU output and the proj / fc2 weights rounded to bf16; the residual stream rounded to f32.
Not mirrored: f32 accumulation order inside an MFMA chain, v_exp_f32 / v_rcp_f32 / the fitted GELU (all around 1e-7 relative, far
below bf16's 2^-9), LayerNorm statistics in f32.  Where that matters the measured factor shows it (FACTORS below).
For tests/bf16_mlp_budget.py (the MLP chain's budget) ``run`` also takes a per-stage ``hook``, ``fresh`` (every bf16 copy centred on the row's
own mean) and the mode "unfolded" (VB_LN_FOLD=0: the LayerNorm in full, its output to bf16, W to bf16 without fold or centring); none of them
changes what it returns without them.

Regimes (``regime``): functions of (name, L, seed) returning the state dict and the fp32 tokens.  Base: synth_vitb_state_dict(seed),
tokens RandomState(1).standard_normal; a zero-mean unit token direction u and a unit direction d_h per head.  The ramp and hot-key
regimes add TOK_AMP a_j u to token j, K_AMP d_h u^T to head h's rows of W_k and Q_AMP d_h (hot keys: HOT_Q d_h) to head h's q bias:
logit_ij gains a per-key term growing with a_j.  The property of each is asserted in fp64 by tests/test_bf16_budget.py, whose docstring
holds the measured values:

  plain        as it is                                        none (logit spread ~13; the running maximum moves 1.3 times in 4 / 2.0 in 11)
  peaked       q, k rows of qkv weight and bias x 3             the largest per-row logit spread is >= 100
  ramp_up      a_j = j / 64                                     the 64-key running maximum moves at every chunk boundary
  ramp_down    a_j = (L - 1 - j) / 64                           it never moves after chunk 0
  last_keys    a_j = HOT_A for the last 8 keys only             the argmax lies in the last 16 keys (704..719 at 720: the real half of the partial
                                                                chunk); the hot logits clear every other key by > 88.7, f32 exp's overflow
  first_keys   a_j = HOT_A for keys 0..7 only                   the same at the other end, in another lane group (added for lane_group_max)
  below_zero   q bias +BZ_AMP d_h, k bias -BZ_AMP d_h           every real logit <= -20: a zero K row (a pad key) would win the softmax
  common_mode  common_mode = 6.0: the tokens ride on +6         none

Which emulated defect (``DEFECTS``, ``attention(..., defect=)``) fails the budget in which regime is the table in the docstring of
tests/test_bf16_budget.py; ``CATCHES`` below is that table as data.  tests/test_gpu_bf16_budget.py runs every regime on every route, so for
a defect d in a route r the failing tests are test_attention_alone[r-<regime>] for the regimes of CATCHES[d].

The width is a parameter: ``regime``, ``attn_only``, ``qkv``, ``logits``, ``run``, ``judge`` (and ``_slots``) take ``w`` = a ``Width`` (C, heads)
of ``WIDTHS`` -- 1024 / 16, 768 / 12, 384 / 6, 192 / 3, 64 columns per head at each; ``attention`` reads it off q.  The default is ViT-Base,
``W768``, and the module-level C, HEADS and amplitudes are its values, so tests/ce_budget.py and the ViT-Base modules use it as before.  The
ramp and hot-key amplitudes depend on the width (``AMPS`` below, with the reason and the measured properties); FACTORS and KO_FRAC do not:
the ratio is against the oracle at the same width, so a correct kernel sits at x1.0 at any width.  tests/test_gpu_bf16_budget_widths.py runs
the routes at the three other widths.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

C, HEADS, HD = 768, 12, 64
Width = namedtuple("Width", "C heads")             # every function below takes w = a Width; the default is ViT-Base
W768 = Width(C, HEADS)
WIDTHS = {1024: Width(1024, 16), 768: W768, 384: Width(384, 6), 192: Width(192, 3)}          # HD = 64 at every one
GEOS = {320: (64, 256), 720: (144, 576)}          # tokens -> (template, search) tokens
SIZES = {320: (128, 256), 720: (192, 384)}        # tokens -> (template, search) pixels
LN_EPS = 1e-6
KC = 64                                            # keys per chunk of vbs::attn_stream_kernel
EPS32 = 2.0 ** -23
FLOOR_ULPS = 0.5

REGIMES = ("plain", "peaked", "ramp_up", "ramp_down", "last_keys", "first_keys", "below_zero", "common_mode")
FULL_REGIMES = ("plain", "peaked", "common_mode", "ramp_up")
TOK_AMP, K_AMP, Q_AMP = 6.0, 2.0, 12.0
HOT_A, HOT_Q = 8.0, 24.0                            # last_keys / first_keys: every query's hot logits clear the rest by > 88.7 = ln(f32 max)
BZ_AMP = 20.0                                      # b_q . b_k / 8 = -50; the cross terms' 5.5 sigma stay below +30

# Per-width amplitudes of the ramp and hot-key regimes.  The LayerNorm in front of qkv turns a token component A u in a row of norm
# ~sqrt(C) into A / sqrt(1 + A^2 / C), which saturates at sqrt(C): with the 768 amplitudes the narrow widths lose the properties (smallest
# hot gap 42-46 at 192, 60-61 at 384; ramp_up 720 moves 8.6 of 11 and ramp_down never moves for only 0.40 at 192).  So the token amplitude
# scales as sqrt(C / 768) and the W_k amplitude as sqrt(768 / C) (the key-side gain K_AMP u . LN(x) then is the 768 one), and HOT_Q is
# raised per width until the smallest hot gap over both frames, all heads and both geometries is >= 95, six units clear of
# ln(f32 max) = 88.73.  Row 768 is the constants above, exactly.  peaked, below_zero, plain and common_mode use none of these (peaked spread
# >= 108, below_zero logits <= -26 at every width).  Measured in fp64 (seed 26, B = 2; tests/test_bf16_budget.py asserts them), at 320 / 720:
#   width   TOK_AMP   K_AMP   HOT_Q   ramp_up moves: all (320) / mean of 11 (720)   ramp_down never moves   smallest hot gap last_keys; first_keys
#   1024    6.93      1.73    26      1.00 / 10.19                                  1.00 / 0.95             107.0 / 97.4;  105.9 / 98.3
#    768    6         2       24      1.00 / 10.28                                  1.00 / 0.94              94.3 / 92.2;   95.6 / 94.3
#    384    4.24      2.83    28      1.00 / 10.14                                  1.00 / 0.99              96.4 / 101.4; 100.1 / 99.2
#    192    3         4       29      1.00 / 10.27                                  1.00 / 0.95             109.3 / 102.2; 103.3 / 96.5
# (With the scaled TOK_AMP / K_AMP and HOT_Q = 24 the smallest gap is 88.1 / 81.0 / 77.5 at 1024 / 384 / 192; it grows by 3.8-4.7 per unit
# of HOT_Q, so one unit below the table's value is under 95 at each.  The 768 row's gaps are what the synthetic weights give it today; they
# are above 88.73, which is what is asserted, and the row is not touched.)
_R = {c: (c / 768.0) ** 0.5 for c in WIDTHS}
AMPS = {c: {"TOK_AMP": TOK_AMP * _R[c], "K_AMP": K_AMP / _R[c], "Q_AMP": Q_AMP, "HOT_A": HOT_A, "HOT_Q": hq, "BZ_AMP": BZ_AMP}
        for c, hq in ((1024, 26.0), (768, HOT_Q), (384, 28.0), (192, 29.0))}
assert AMPS[768] == {"TOK_AMP": TOK_AMP, "K_AMP": K_AMP, "Q_AMP": Q_AMP, "HOT_A": HOT_A, "HOT_Q": HOT_Q, "BZ_AMP": BZ_AMP}

# error(kernel) / error(bf16 oracle) allowed, for rel-L2, max-abs and the worst (frame, head, 16-query tile) slot's rel-L2.  Set from ONE
# MI355X run of tests/test_gpu_bf16_budget.py's cases, each against the oracle (never against the kernel's own output), as 1.5 x the worst
# ratio seen over routes and regimes; the cap, a third of the smallest ratio a defect reaches in a catching regime (x26: swap4_v in
# peaked, max-abs; tests/test_bf16_budget.py), is far away.  Measured, rel-L2 / max-abs / worst slot [kernel - oracle as a fraction of
# the oracle's error]:
#   attention alone   fused = unfused   every regime x1.00 / x1.00 / x1.01-1.03, below_zero slot x1.10       [0.01-0.06, common_mode 0.22]
#                     stream320         every regime x1.00 / x1.00 / x1.01-1.04, below_zero slot x1.09       [0.01-0.06, common_mode 0.22]
#                     stream720         every regime x1.00 / x1.00 / x1.01-1.06 (peaked 1.06, common_mode 1.05), each frame of every
#                                       regime on its own the same                                            [0.02-0.09, common_mode 0.23]
#   after 1 block     all routes        x1.00 / x0.94-1.03 / x1.00-1.05                                       [0.03-0.19, common_mode 0.41]
#   after 2 blocks    all routes        x1.00 / x0.82-1.09 / x1.03-1.09                                       [0.14-0.65, common_mode 0.71]
# No route or regime stands out: the kernels' error IS the oracle's (the one earlier hardware data point, 1.16e-3 against 1.17e-3 on a
# plain block, said the same).  common_mode's larger kernel-oracle distance: the device centres its bf16 copy on an f32 mean, the oracle
# on the fp64 one, and at |x| ~ 6 that moves more rounding boundaries; both sit at x1.00 of the truth.
FACTORS = {"attn": 1.65, "resid1": 1.6, "resid2": 1.65}

# kernel - oracle, rel-L2 as a fraction of the oracle's own error against the truth: the sharpest figure here, the two differing only by
# bf16 rounding-boundary flips and summation order.  On attention alone it was <= 0.23 in every route and regime, stably below half, so it
# is asserted at 3 x that.  After whole blocks it is NOT asserted: it reaches 0.41 after one block and 0.71 after two (flips compound
# through fc1 / GELU / fc2 and the next block's LayerNorm while both stay at x1.00 of the truth), which is not below half.
KO_FRAC = {"attn": 0.69}

# which regimes must fail each emulated defect (tests/test_bf16_budget.py asserts exactly this, at the geometry named)
CATCHES = {
    "no_O_rescale": {320: ("plain", "peaked", "ramp_up"), 720: ("ramp_up",)},
    "no_l_rescale": {320: ("ramp_up",), 720: ("ramp_up",)},
    "lane_group_max": {320: ("last_keys", "first_keys"), 720: ("last_keys", "first_keys")},
    "pad_leak": {720: ("below_zero",)},
    "pad_v_nan": {720: ("plain", "peaked", "below_zero")},
    "drop_last16": {320: ("last_keys",), 720: ("last_keys",)},
    "swap4_v": {320: ("plain", "peaked"), 720: ("plain",)},
    "no_log2e": {320: ("plain",), 720: ("plain",)},
    "head_shift": {320: ("plain",), 720: ("plain",)},
}
DEFECTS = tuple(CATCHES)
STREAM_DEFECTS = ("no_O_rescale", "no_l_rescale")      # emulated in the 64-key chunked form


def bf16(a):
    """Round-to-nearest-even bf16 of a float array, returned as float64 (torch does the rounding, as in tests/vitb_u8_fold.py)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- regimes
def _ramp(name, L, hot_a=HOT_A):
    j = np.arange(L, dtype=np.float64)
    if name == "ramp_up":
        return j / KC
    if name == "ramp_down":
        return (L - 1 - j) / KC
    if name == "last_keys":
        return np.where(j >= L - 8, hot_a, 0.0)
    if name == "first_keys":
        return np.where(j < 8, hot_a, 0.0)
    return None


def regime(name, L, seed=26, B=2, depth=1, w=W768):
    """(state dict, fp32 tokens (B, L, C)) of regime `name` at L = 320 or 720 tokens and width w, at that width's amplitudes (AMPS)."""
    from vittracker_amd import synth
    assert name in REGIMES, name
    C, HEADS = w
    TOK_AMP, K_AMP, Q_AMP, HOT_A, HOT_Q, BZ_AMP = (AMPS[C][k] for k in ("TOK_AMP", "K_AMP", "Q_AMP", "HOT_A", "HOT_Q", "BZ_AMP"))
    lz, lx = GEOS[L]
    cm = 6.0 if name == "common_mode" else 0.0
    sd = synth.synth_vitb_state_dict(seed, C=C, depth=depth, heads=HEADS, len_z=lz, len_x=lx, common_mode=cm)
    X = np.random.RandomState(1).standard_normal((B, L, C)) + cm
    rs = np.random.RandomState(1000 + seed)
    u = rs.standard_normal(C)
    u -= u.mean()
    u /= np.linalg.norm(u)
    d = rs.standard_normal((HEADS, HD))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = _ramp(name, L, HOT_A)
    if a is not None:
        X += TOK_AMP * a[None, :, None] * u
    for i in range(depth):
        p = f"backbone.blocks.{i}.attn.qkv."
        W, b = sd[p + "weight"].astype(np.float64), sd[p + "bias"].astype(np.float64)
        if name == "peaked":
            W[:2 * C] *= 3.0
            b[:2 * C] *= 3.0
        if a is not None:
            W[C:2 * C] += K_AMP * np.einsum("hd,c->hdc", d, u).reshape(C, C)
            b[:C] += (HOT_Q if name in ("last_keys", "first_keys") else Q_AMP) * d.reshape(C)
        if name == "below_zero":
            b[:C] += BZ_AMP * d.reshape(C)
            b[C:2 * C] -= BZ_AMP * d.reshape(C)
        sd[p + "weight"], sd[p + "bias"] = W.astype(np.float32), b.astype(np.float32)
    return sd, X.astype(np.float32)


def attn_only(sd, i=0, w=W768):
    """A copy of `sd` whose block i returns x + attention(x): proj = identity, proj.bias = 0, fc2 = 0."""
    sd = dict(sd)
    C = w.C
    p = f"backbone.blocks.{i}."
    sd[p + "attn.proj.weight"] = np.eye(C, dtype=np.float32)
    sd[p + "attn.proj.bias"] = np.zeros(C, np.float32)
    sd[p + "mlp.fc2.weight"] = np.zeros_like(sd[p + "mlp.fc2.weight"])
    sd[p + "mlp.fc2.bias"] = np.zeros(C, np.float32)
    return sd


# ----------------------------------------------------------------------------- the block, truth and oracle
def _w(sd, name):
    return np.asarray(sd[name], np.float64)


def _stats(x):
    mean = x.mean(-1)
    xc = x - mean[..., None]
    return mean, xc, 1.0 / np.sqrt((xc * xc).mean(-1) + LN_EPS)


def fold(W, b, g, be, nscaled=0):
    """vitb.hip fold_layernorm + the attention scale: (bf16(W') as float64, b' as f32 in float64)."""
    Wg = W * g
    Wf = (Wg - Wg.mean(1, keepdims=True)).astype(np.float32)
    bf_ = (b + W @ be).astype(np.float32)
    Wf[:nscaled] *= np.float32(0.125)
    bf_[:nscaled] *= np.float32(0.125)
    return bf16(Wf), bf_.astype(np.float64)


def _linear_ln(sd, p, ln, lin, x, mode, centre, nscaled=0, rstd=None):
    """LayerNorm `ln` + Linear `lin` of block prefix p on rows x: fp64 as the reference writes it, folded on bf16 operands ('bf16'), or
    -- mode 'unfolded', VB_LN_FOLD=0 -- the LayerNorm applied in full, its output rounded to bf16, W rounded to bf16 without fold or
    centring.  rstd: stands in for the rows' own 1 / sqrt(var + eps) in the folded form (tests/bf16_mlp_budget.py emulates defects of
    the statistics with it)."""
    W, b, g, be = _w(sd, p + lin + ".weight"), _w(sd, p + lin + ".bias"), _w(sd, p + ln + ".weight"), _w(sd, p + ln + ".bias")
    mean, xc, rstd_x = _stats(x)
    if mode == "truth":
        y = (xc * rstd_x[..., None] * g + be) @ W.T + b
        y[..., :nscaled] *= 0.125
        return y
    if mode == "unfolded":
        y = bf16(xc * rstd_x[..., None] * g + be) @ bf16(W).T + b
        y[..., :nscaled] *= 0.125
        return y
    Wf, bf_ = fold(W, b, g, be, nscaled)
    xb = bf16(x - (mean if centre is None else centre)[..., None])
    return (xb @ Wf.T) * (rstd_x if rstd is None else rstd)[..., None] + bf_


def qkv(sd, x, i=0, mode="truth", centre=None, w=W768, rstd=None):
    """q (scaled by 1/8), k, v of block i as (B, heads, L, 64) float64; bf16 values in mode 'bf16' / 'unfolded'."""
    y = _linear_ln(sd, f"backbone.blocks.{i}.", "norm1", "attn.qkv", np.asarray(x, np.float64), mode, centre, nscaled=w.C, rstd=rstd)
    if mode != "truth":
        y = bf16(y)
    B, L = y.shape[:2]
    y = y.reshape(B, L, 3, w.heads, HD).transpose(2, 0, 3, 1, 4)
    return y[0], y[1], y[2]


def logits(sd, X, i=0, w=W768):
    """The fp64 logits (B, heads, L, L) of block i on tokens X."""
    q, k, _ = qkv(sd, X, i, "truth", w=w)
    return q @ k.transpose(0, 1, 3, 2)


def hot_group(L):
    """The lane group (key % 32) // 8 that holds the eight hot keys of last_keys: 3 at 320 tokens, 1 at 720 (first_keys: group 0)."""
    return ((L - 8) % 32) // 8


def attention(q, k, v, mode="truth", chunk=None, defect=None, group=0):
    """softmax(q k^T) v per (frame, head) -> (B, L, heads x 64), the width read off q.  mode 'bf16' rounds P for P.V (row sum from the
    unrounded P) and the output; chunk = 64 runs the online softmax of the streaming kernel.  defect: one of DEFECTS, emulated on top of
    the bf16 oracle."""
    B, H, L, _ = q.shape
    rnd = bf16 if mode != "truth" else (lambda a: a)
    real = np.ones(k.shape[2], bool)                    # keys whose score is not masked
    if defect == "head_shift":                          # q, k of head h with v of head (h + 1) mod heads: a wrong section distance or
        v = np.roll(v, -1, axis=1)                      # head-group stride on ONE operand
    if defect in ("pad_leak", "pad_v_nan"):             # 16 keys past the frame in the last 32-key chunk: K rows zero (the workspace tail)
        vpad = np.roll(v, 1, axis=0)[:, :, :16] if defect == "pad_leak" else np.full_like(v[:, :, :16], np.nan)
        k = np.concatenate([k, np.zeros_like(k[:, :, :16])], axis=2)
        v = np.concatenate([v, vpad], axis=2)
        real = np.concatenate([real, np.full(16, defect == "pad_leak")])
    if defect == "drop_last16":
        k, v, real = k[:, :, :L - 16], v[:, :, :L - 16], real[:L - 16]
    if defect == "swap4_v":                             # keys j and j ^ 4 exchanged on the V^T side only
        v = v[:, :, np.arange(L) ^ 4]
    if defect in STREAM_DEFECTS and chunk is None:
        chunk = KC
    ex = np.exp2 if defect == "no_log2e" else np.exp
    out = np.empty((B, L, H * HD))
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            S = q[b] @ k[b].transpose(0, 2, 1)
            S[..., ~real] = -np.inf
            if defect == "lane_group_max":              # the maximum of the keys of ONE lane group, applied to the whole row; exp in f32
                grp = (np.arange(S.shape[-1]) % 32) // 8 == group
                P = np.exp((S - S[..., grp].max(-1, keepdims=True)).astype(np.float32)).astype(np.float64)
                O = (rnd(P) @ v[b]) / P.sum(-1, keepdims=True)
            elif chunk is None:
                P = ex(S - S.max(-1, keepdims=True))
                O = (rnd(P) @ v[b]) / P.sum(-1, keepdims=True)
            else:
                m = np.full(S.shape[:2] + (1,), -1e30)
                l = np.zeros_like(m)
                O = np.zeros(S.shape[:2] + (HD,))
                for c in range(0, S.shape[-1], chunk):
                    Sc = S[..., c:c + chunk]
                    mx = np.maximum(m, Sc.max(-1, keepdims=True))
                    alpha = ex(m - mx)
                    P = ex(Sc - mx)
                    l = l * (1.0 if defect == "no_l_rescale" else alpha) + P.sum(-1, keepdims=True)
                    O = O * (1.0 if defect == "no_O_rescale" else alpha) + rnd(P) @ v[b][:, c:c + chunk]
                    m = mx
                O = O / l
            out[b] = rnd(O).transpose(1, 0, 2).reshape(L, H * HD)
    return out


def run(sd, X, nblocks=1, mode="truth", chunk=None, w=W768, hook=None, fresh=False):
    """[residual after block 1 .. nblocks] (f32 values in mode 'bf16' / 'unfolded') and block 0's attention output, from fp32 tokens X.
    hook(i, stage, value): called per block i at the stages "ao" (attention output), "x1" (residual after proj), "u" (fc1 pre-activation),
    "h" (hidden activations, after the GELU and its rounding) and "x" (residual after fc2); what it returns, unless None, replaces the
    value.  In the folded oracle it is also asked for "rstd1" / "rstd2" with the rows norm1 / norm2 see: an array returned stands in for
    their rstd.  fresh: the oracle centres every bf16 copy on the row's OWN mean, where the device uses the mean from before the last
    update (tests/bf16_mlp_budget.py measures the difference)."""
    def tap(i, stage, v):
        r = None if hook is None else hook(i, stage, v)
        return v if r is None else r

    def ask(i, stage, v):
        return None if hook is None or mode != "bf16" else hook(i, stage, v)

    x = np.asarray(X, np.float64)
    res, ao0, centre = [], None, None
    gelu = lambda u: 0.5 * u * (1.0 + _erf(u / np.sqrt(2.0)))
    for i in range(nblocks):
        p = f"backbone.blocks.{i}."
        ao = attention(*qkv(sd, x, i, mode, centre, w=w, rstd=ask(i, "rstd1", x)), mode=mode, chunk=chunk)
        ao = tap(i, "ao", ao)
        ao0 = ao if i == 0 else ao0
        if mode == "truth":
            x1 = tap(i, "x1", x + ao @ _w(sd, p + "attn.proj.weight").T + _w(sd, p + "attn.proj.bias"))
            h = tap(i, "h", gelu(tap(i, "u", _linear_ln(sd, p, "norm2", "mlp.fc1", x1, mode, None))))
            x = tap(i, "x", x1 + h @ _w(sd, p + "mlp.fc2.weight").T + _w(sd, p + "mlp.fc2.bias"))
        else:
            c0 = x.mean(-1) if centre is None else centre                 # what the proj GEMM centres its bf16 copy on
            x1 = tap(i, "x1", f32(x + ao @ bf16(_w(sd, p + "attn.proj.weight")).T + _w(sd, p + "attn.proj.bias")))
            c0 = x1.mean(-1) if fresh else c0
            h = tap(i, "u", _linear_ln(sd, p, "norm2", "mlp.fc1", x1, mode, c0, rstd=ask(i, "rstd2", x1)))
            h = tap(i, "h", bf16(gelu(h)))
            x = tap(i, "x", f32(x1 + h @ bf16(_w(sd, p + "mlp.fc2.weight")).T + _w(sd, p + "mlp.fc2.bias")))
            centre = x.mean(-1) if fresh else x1.mean(-1)                 # ... and the fc2 GEMM: the mean ln_finalize found after proj
        res.append(x)
    return res, ao0


def _erf(a):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


# ----------------------------------------------------------------------------- regime properties (fp64)
def chunk_moves(S):
    """Per (frame, head, query): at how many of the chunk boundaries the running maximum of the 64-key chunks moves."""
    n = -(-S.shape[-1] // KC)
    cm = np.stack([S[..., c * KC:(c + 1) * KC].max(-1) for c in range(n)], -1)
    run_ = np.maximum.accumulate(cm, -1)
    return (cm[..., 1:] > run_[..., :-1]).sum(-1), n - 1


def properties(S):
    """What tests/test_bf16_budget.py asserts and NOTES.md records, from the fp64 logits S (B, heads, L, L)."""
    L = S.shape[-1]
    moves, nb = chunk_moves(S)
    P = np.exp(S - S.max(-1, keepdims=True))
    srt = np.sort(S, -1)
    return {"hot_gap": float((srt[..., -8] - srt[..., -9]).min()), "argmax_first16": float((S.argmax(-1) < 16).mean()),
            "spread": float((S.max(-1) - S.min(-1)).max()), "top_p": float((1.0 / P.sum(-1)).mean()), "boundaries": nb,
            "moves_mean": float(moves.mean()), "moves_all": float((moves == nb).mean()), "moves_none": float((moves == 0).mean()),
            "argmax_last16": float((S.argmax(-1) >= L - 16).mean()), "max_logit": float(S.max()),
            "below_m20": float((S <= -20.0).mean())}


# ----------------------------------------------------------------------------- the budget
def _slots(a, w=W768):
    """(B, L, C) -> (B, heads, L / 16, 16 x 64): one row per (frame, head or 64-column slice, 16-query tile)."""
    B, L, _ = a.shape
    return a.reshape(B, L // 16, 16, w.heads, HD).transpose(0, 3, 1, 2, 4).reshape(B, w.heads, L // 16, 16 * HD)


def errors(got, truth, denom=None):
    """(rel-L2, max-abs) of `got` against `truth`; rel-L2 against ||denom|| (default: ||truth||)."""
    d = np.asarray(got, np.float64) - truth
    den = truth if denom is None else denom
    return float(np.linalg.norm(d) / max(np.linalg.norm(den), 1e-300)), float(np.abs(d).max())


def judge(stage, kernel, truth, oracle, factor=None, at=None, centred=False, w=W768):
    """One stage on (B, L, C) arrays of width w: the kernel's and the oracle's rel-L2 and max-abs against the truth, the bounds
    factor * oracle + floor, and the same for every (frame, head, 16-query tile) slot's rel-L2, of which the worst ratio and its slot
    are returned; with the stage's own factor the kernel - oracle distance is held to KO_FRAC[stage] of the oracle's error too.  at: the values at whose magnitude the observed quantity was rounded to f32 (default: the truth itself);
    centred: rel-L2 against the rows' centred norm (what a LayerNorm sees, vitb_u8_fold.rel_c)."""
    f = FACTORS[stage] if factor is None else factor
    kernel, truth, oracle = (np.asarray(a, np.float64) for a in (kernel, truth, oracle))
    assert kernel.shape == truth.shape == oracle.shape and kernel.shape[-1] == w.C, (kernel.shape, truth.shape, oracle.shape, w)
    at = truth if at is None else np.asarray(at, np.float64)
    den = truth - truth.mean(-1, keepdims=True) if centred else truth
    k_rel, k_abs = errors(kernel, truth, den)
    o_rel, o_abs = errors(oracle, truth, den)
    fl_rel = FLOOR_ULPS * EPS32 * float(np.linalg.norm(at) / max(np.linalg.norm(den), 1e-300))
    fl_abs = FLOOR_ULPS * EPS32 * float(np.abs(at).max())
    b_rel, b_abs = f * o_rel + fl_rel, f * o_abs + fl_abs
    sden = np.maximum(np.linalg.norm(_slots(den, w), axis=-1), 1e-300)
    sk = np.linalg.norm(_slots(kernel - truth, w), axis=-1) / sden
    so = np.linalg.norm(_slots(oracle - truth, w), axis=-1) / sden
    sfl = FLOOR_ULPS * EPS32 * np.linalg.norm(_slots(at, w), axis=-1) / sden
    with np.errstate(invalid="ignore"):
        excess = np.where(np.isfinite(sk), sk / (f * so + sfl), np.inf)      # > 1: the slot is over its bound
        ratio = np.where(np.isfinite(sk), sk / np.maximum(so, 1e-300), np.inf)
    worst = np.unravel_index(int(np.argmax(excess)), excess.shape)
    ko = errors(kernel, oracle, den)[0]
    finite = bool(np.isfinite(kernel).all())
    return {"stage": stage, "kernel_rel": k_rel, "kernel_abs": k_abs, "oracle_rel": o_rel, "oracle_abs": o_abs,
            "bound_rel": b_rel, "bound_abs": b_abs, "ratio_rel": k_rel / max(o_rel, 1e-300), "ratio_abs": k_abs / max(o_abs, 1e-300),
            "slot": tuple(int(i) for i in worst), "slot_ratio": float(ratio.max()), "slot_excess": float(excess.max()),
            "ko_rel": ko, "ko_frac": ko / max(o_rel, 1e-300), "finite": finite,
            "ok": finite and k_rel <= b_rel and k_abs <= b_abs and float(excess.max()) <= 1.0
                  and (factor is not None or ko <= KO_FRAC.get(stage, np.inf) * o_rel + fl_rel)}


def fmt(r):
    return (f"{r['stage']:>28}: rel {r['kernel_rel']:.2e} (oracle {r['oracle_rel']:.2e}, x{r['ratio_rel']:.2f}, bound {r['bound_rel']:.2e})"
            f"  abs {r['kernel_abs']:.2e} (oracle {r['oracle_abs']:.2e}, x{r['ratio_abs']:.2f}, bound {r['bound_abs']:.2e})"
            f"  worst slot (frame, head, tile) {r['slot']} x{r['slot_ratio']:.2f}  kernel-oracle {r['ko_rel']:.2e} = {r['ko_frac']:.2f} of the oracle's"
            + ("" if r["ok"] else "  OVER"))
