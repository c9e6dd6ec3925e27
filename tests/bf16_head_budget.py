"""The bf16 accuracy budget of the ViT box head (vb::head in vitb.hip: feat_to_map_kernel, the three conv towers as implicit GEMMs --
vbg::A_CONV / EPI_CONV in vb_gemm.h -- and conv5_kernel): a kernel's error against the fp64 truth, held to a multiple of the error of an
oracle that rounds to bf16 where the device does, on the same features -- per feature regime, per map, per (frame, output channel).

A plain helper for tests/test_bf16_head_budget.py (CPU: the regimes have the stated properties, the budget has teeth) and
tests/test_gpu_bf16_head_budget.py (the head on the device at four widths, two map sizes and both tile forms), modelled on
tests/bf16_budget.py and tests/fp32_budget.py.

Truth and oracle (``head``): (B, F^2, C) fp32 features -> {"score_map" (B, 1, F, F), "size_map" (B, 2, F, F), "offset_map" (B, 2, F, F)} as
float64, in plain numpy: every 3 x 3 conv is nine shifted matmuls over a zero-bordered (F + 2)^2 NHWC array.
  truth   fp64 throughout: conv + bias, BatchNorm(eval, eps 1e-5) as the reference's head writes it, ReLU, four times per tower; a 1 x 1 conv;
          sigmoid and clamp to [1e-4, 1 - 1e-4] on ctr and size.
  bf16    * the features rounded to bf16 (feat_to_map_kernel; the final-LayerNorm kernel writes the same map from the same f32 values);
          * BN folded as vitb.hip's loader does: k = g / sqrt(var + 1e-5), W' = W k, b' = (b - mu) k + beta in double, both through f32, W'
            then to bf16, b' staying f32;
          * every tower layer's output bf16(relu(acc + b'));
          * conv5 with its f32 weights, unrounded, on the bf16 map; the maps rounded to f32.
Not mirrored: f32 accumulation order inside the MFMA chain (the oracle accumulates in fp64), expf in the sigmoid, conv5_kernel's fmaf
order, the clamp constants as f32 -- all around 1e-7 relative, far below bf16's 2^-9.  Where that matters the measured factor shows it.

Regimes (``regime(name, B, F, C, seed)`` -> fp32 features; the property of each is asserted in fp64 by tests/test_bf16_head_budget.py):
  plain          unit-normal rows -- what the final LayerNorm delivers
  one_token      zero except ONE search token per frame (|value| in [0.5, 1.5], random signs); frame i takes pixel i of ``pixels(F)``: the
                 four corners, one pixel on each edge, one interior pixel.  Its 3 x 3 footprints grow layer by layer into the borders.
                 Property: the truth's maps differ from the all-zero-feature maps exactly on the 9 x 9 window round the token (clipped to
                 the map) -- the receptive field, hence tap order and borders.
  edge_hot       unit-normal x EDGE_AMP on the outer ring of pixels, x 0.25 inside.  Property: >= 60 % of the feature energy in the ring.
  frames_differ  plain, frame b scaled by 1 + FRAME_STEP b.  Property: no two frames' truth maps are within 10 x the oracle's error of each
                 other, so a frame mix-up cannot pass.
The state dict is synth.synth_vitb_state_dict(seed 26) at the width (``state``), the same for every regime and map size.

Emulated defects (``DEFECTS``, ``head(..., defect=)``, on top of the bf16 oracle) and the regimes that must fail each (``CATCHES``): the table
is in the docstring of tests/test_bf16_head_budget.py.  ``batch``: the frames of one launch -- the tile defects (straddle, droptail) depend on
M = batch x F^2; nine one_token frames run as launches of ``batch`` frames.

Amplitudes.  With edge_hot at x 4 and frames_differ at 1 + b the truth alone puts more than 1 % of the score / size values on the sigmoid
clamp (seed 26: edge_hot 2.0 % at width 384 / F = 16; frames_differ 5.4 % at 192 / 24, still 1.6 % at 1 + b / 2), where a kernel's error
vanishes and the budget says nothing.  With EDGE_AMP = 3 and FRAME_STEP = 0.25 every regime, width and map size stays inside 1 % (the
largest share: 0.98 % at 384 / 16 edge_hot, then 0.29 %; plain <= 0.02 %, one_token 0) -- tests/test_bf16_head_budget.py asserts it.
"""
from __future__ import annotations

import numpy as np

from bf16_budget import EPS32, FLOOR_ULPS, WIDTHS, bf16, f32

MAPS = ("score_map", "size_map", "offset_map")
TOWERS = ("ctr", "offset", "size")
HEAD_CH = 256
BN_EPS = 1e-5
CLAMP_LO, CLAMP_HI = 1e-4, 1.0 - 1e-4
SEED = 26
GEOMS = {16: (128, 256, 2), 24: (192, 384, 3)}          # F -> (template px, search px, frames of a launch in the GPU module)
REGIMES = ("plain", "one_token", "edge_hot", "frames_differ")
EDGE_AMP, EDGE_IN = 3.0, 0.25
FRAME_STEP = 0.25
TILE_M = 256                                            # rows of the widest GEMM tile


def pixels(F):
    """(row, column) of the one live token of one_token's frame i: four corners, one pixel on each edge, one interior pixel."""
    return [(0, 0), (0, F - 1), (F - 1, 0), (F - 1, F - 1), (0, 3), (F // 2, 0), (F - 1, F - 3), (2, F - 1), (F // 2 - 1, F // 2)]


def state(C, F=16, seed=SEED):
    """The synthetic depth-1 state dict of width C at map size F (the head's weights do not depend on F; the position embeddings do)."""
    from vittracker_amd import synth
    return synth.synth_vitb_state_dict(seed, C=C, depth=1, heads=WIDTHS[C].heads, len_z=(F // 2) ** 2, len_x=F * F)


def regime(name, B, F, C, seed=SEED):
    """fp32 features (B, F^2, C) of regime `name`."""
    assert name in REGIMES, name
    rs = np.random.RandomState(7000 + seed)
    if name == "one_token":
        px = pixels(F)
        X = np.zeros((B, F * F, C))
        for i in range(B):
            y, x = px[i % len(px)]
            X[i, y * F + x] = rs.uniform(0.5, 1.5, C) * rs.choice([-1.0, 1.0], C)
        return X.astype(np.float32)
    X = rs.standard_normal((B, F * F, C))
    if name == "edge_hot":
        X *= np.where(ring(F), EDGE_AMP, EDGE_IN).reshape(1, F * F, 1)
    if name == "frames_differ":
        X *= (1.0 + FRAME_STEP * np.arange(B)).reshape(B, 1, 1)
    return X.astype(np.float32)


def ring(F):
    """(F, F) bool: the outer ring of pixels."""
    r = np.zeros((F, F), bool)
    r[0], r[-1], r[:, 0], r[:, -1] = True, True, True, True
    return r


# ----------------------------------------------------------------------------- the head, truth and oracle
# defect -> {F: regimes that must fail it}.  Every defect is visible in every regime (measured ratios: tests/test_bf16_head_budget.py), save
# the two tile defects at F = 16, where M = B x 256 is a multiple of the tile and they change nothing: the reason F = 24 is run.
_ALL = {16: REGIMES, 24: REGIMES}
CATCHES = {
    "tower_w2": _ALL,          # conv2 weights of the offset and size towers exchanged (gW)
    "bias0_l2": _ALL,          # conv2 of every tower takes tower 0's bias (gBias)
    "norelu4": _ALL,           # no ReLU after conv4
    "taps_T": _ALL,            # conv1's taps transposed, (r, s) <-> (s, r)
    "edge_l1": _ALL,           # layer li reads a replicated border instead of zero
    "edge_l2": _ALL,
    "edge_l3": _ALL,
    "edge_l4": _ALL,
    "w5swap": _ALL,            # conv5's two offset rows exchanged
    "pad32": _ALL,             # the last 8 of conv4's 32 columns never written
    "straddle": {16: (), 24: REGIMES},          # conv4's rows past a frame boundary inside a 256-row tile not written
    "droptail": {16: (), 24: REGIMES},          # conv4's last, partial 256-row tile not written
}
DEFECTS = tuple(CATCHES)
_FIRST = {"tower_w2": 2, "bias0_l2": 2, "norelu4": 4, "taps_T": 1, "edge_l1": 1, "edge_l2": 2, "edge_l3": 3, "edge_l4": 4, "w5swap": 5,
          "pad32": 5, "straddle": 5, "droptail": 5}          # the first layer a defect changes (5: behind the towers)


def _w(sd, name):
    return np.asarray(sd[name], np.float64)


def _layer(sd, t, li, mode):
    """(W (cout, cin, 3, 3), b (cout,), bn) of conv li (1..4) of tower t: as the reference holds them (bn = (g, beta, mu, var)), or
    folded and rounded as vitb.hip's loader leaves them (bn = None)."""
    p = f"box_head.conv{li}_{t}."
    W, b = _w(sd, p + "0.weight"), _w(sd, p + "0.bias")
    g, beta, mu, var = (_w(sd, p + "1." + k) for k in ("weight", "bias", "running_mean", "running_var"))
    if mode == "truth":
        return W, b, (g, beta, mu, var)
    k = g / np.sqrt(var + BN_EPS)
    return bf16(f32(W * k[:, None, None, None])), f32((b - mu) * k + beta), None


def conv3x3(x, W, edge=False):
    """x (B, F, F, cin) -> (B, F, F, cout): nine shifted matmuls over the bordered map (zero border; edge: a replicated one)."""
    B, F, _, cin = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge" if edge else "constant")
    Wt = np.ascontiguousarray(W.transpose(2, 3, 1, 0))          # (r, s, cin, cout): contiguous operands, so that matmul goes to BLAS
    out = np.zeros((B * F * F, W.shape[0]))
    for r in range(3):
        for s in range(3):
            out += np.ascontiguousarray(xp[:, r:r + F, s:s + F, :]).reshape(B * F * F, cin) @ Wt[r, s]
    return out.reshape(B, F, F, -1)


def _unwritten(B, F, defect):
    """(B x F^2,) bool: the rows of one launch of B frames that the tile defect leaves unwritten."""
    M = B * F * F
    m = np.arange(M)
    if defect == "straddle":                    # rows past a frame boundary inside a 256-row tile
        return m // (F * F) > (m // TILE_M * TILE_M) // (F * F)
    return m >= M // TILE_M * TILE_M            # droptail: the last, partial tile


def head(sd, feat, mode="truth", defect=None, batch=None, memo=None):
    """The three maps, float64, from features (B, F^2, C).  mode 'truth' | 'bf16'; defect: one of DEFECTS on top of the bf16 oracle;
    batch: frames of one launch (default: all B); memo: a dict that keeps the defect-free tower layers of this (sd, feat, mode), so
    that a defect's run starts at the first layer it changes."""
    assert mode in ("truth", "bf16") and (defect is None or (defect in DEFECTS and mode == "bf16")), (mode, defect)
    feat = np.asarray(feat)
    B, LX, C = feat.shape
    F = int(round(LX ** 0.5))
    assert F * F == LX
    batch = B if batch is None else batch
    memo = {} if memo is None else memo
    first = _FIRST.get(defect, 99)
    x0 = feat.astype(np.float64).reshape(B, F, F, C)
    if mode == "bf16":
        x0 = bf16(x0)
    t4 = {}
    for t in TOWERS:
        x = x0
        for li in range(1, 5):
            if li < first and (mode, t, li) in memo:
                x = memo[(mode, t, li)]
                continue
            src = {"offset": "size", "size": "offset"}.get(t, t) if (defect == "tower_w2" and li == 2) else t
            W, b, bn = _layer(sd, src, li, mode)
            if src != t or (defect == "bias0_l2" and li == 2):
                b = _layer(sd, "ctr" if defect == "bias0_l2" else t, li, mode)[1]
            if defect == "taps_T" and li == 1:
                W = W.transpose(0, 1, 3, 2)
            y = conv3x3(x, W, edge=defect == f"edge_l{li}") + b
            if bn is not None:
                g, beta, mu, var = bn
                y = (y - mu) / np.sqrt(var + BN_EPS) * g + beta
            if not (defect == "norelu4" and li == 4):
                y = np.maximum(y, 0.0)
            x = bf16(y) if mode == "bf16" else y
            if li < first:
                memo[(mode, t, li)] = x
        if defect == "pad32":                   # the last 8 of conv4's 32 columns never written (the map is zero-filled)
            x = x.copy()
            x[..., 24:] = 0.0
        if defect in ("straddle", "droptail"):
            x = x.reshape(B * LX, -1).copy()
            for b0 in range(0, B, batch):
                nb = min(batch, B - b0)
                x[b0 * LX:(b0 + nb) * LX][_unwritten(nb, F, defect)] = 0.0
            x = x.reshape(B, F, F, -1)
        t4[t] = x
    out = {}
    for t, name in (("ctr", "score_map"), ("size", "size_map"), ("offset", "offset_map")):
        W5, b5 = _w(sd, f"box_head.conv5_{t}.weight").reshape(-1, HEAD_CH // 8), _w(sd, f"box_head.conv5_{t}.bias")
        if defect == "w5swap" and t == "offset":
            W5 = W5[::-1]
        y = (t4[t] @ W5.T + b5).transpose(0, 3, 1, 2)
        if t != "offset":
            y = np.clip(1.0 / (1.0 + np.exp(-y)), CLAMP_LO, CLAMP_HI)
        out[name] = f32(y) if mode == "bf16" else y
    return out


def clamp_share(maps):
    """The share of the score / size values that lie on the sigmoid clamp."""
    v = np.concatenate([maps["score_map"].ravel(), maps["size_map"].ravel()])
    return float(((v <= CLAMP_LO) | (v >= CLAMP_HI)).mean())


# ----------------------------------------------------------------------------- the budget
# error(kernel) / error(bf16 oracle) allowed per map, for rel-L2 and max-abs of the map and of every (frame, output channel) slot.  Set from
# ONE MI355X run of tests/test_gpu_bf16_head_budget.py, each case against the oracle (never against the kernel's own output), as 1.5 x the
# worst ratio seen over all cases and all four figures: score_map x1.12 (1024 / 16 edge_hot, max-abs), size_map x1.47 (1024 / 24 edge_hot, one
# slot's max-abs: one pixel of one channel, the map's rel-L2 at x1.02), offset_map x1.17 (1024 / 24 one_token, one slot's max-abs).  The cap,
# a third of the smallest ratio a defect reaches in a catching regime (x32.9: bias0_l2, frames_differ, 192 / 16;
# tests/test_bf16_head_budget.py), is 10.9 -- five times further out.  Measured, rel-L2 / max-abs / worst slot rel-L2 / worst slot max-abs
# [kernel - oracle as a fraction of the oracle's error], score_map   size_map   offset_map; "default = wide": both forms ran and gave the
# same figures (as the narrow == wide bit-identity tests require):
#   width / F  case                   forms
#   1024 / 16  plain                  default = wide x1.01 / x1.00 / x1.02 / x1.00 [0.18]   x1.01 / x1.00 / x1.02 / x1.00 [0.23]   x0.98 / x1.00 / x1.00 / x1.00 [0.22]
#   1024 / 16  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.02 / x1.00 [0.03]
#   1024 / 16  edge_hot               default        x1.00 / x1.12 / x1.00 / x1.12 [0.16]   x1.01 / x0.94 / x1.02 / x1.00 [0.22]   x1.00 / x1.16 / x1.01 / x1.16 [0.18]
#   1024 / 16  frames_differ          default        x1.00 / x1.00 / x1.02 / x1.00 [0.17]   x1.00 / x0.99 / x1.01 / x1.00 [0.24]   x0.99 / x1.00 / x1.00 / x1.04 [0.18]
#   1024 / 24  plain                  default = wide x1.00 / x0.98 / x1.02 / x1.08 [0.16]   x1.00 / x1.18 / x1.01 / x1.18 [0.22]   x1.00 / x1.00 / x1.01 / x1.00 [0.16]
#   1024 / 24  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.01]   x1.00 / x1.00 / x1.02 / x1.17 [0.06]   x1.00 / x1.00 / x1.01 / x1.17 [0.03]
#   1024 / 24  edge_hot               default        x0.99 / x1.00 / x1.01 / x1.00 [0.16]   x1.02 / x1.05 / x1.09 / x1.47 [0.23]   x1.00 / x1.00 / x1.01 / x1.05 [0.18]
#   1024 / 24  frames_differ          default        x1.00 / x1.00 / x1.01 / x1.00 [0.19]   x0.99 / x1.02 / x1.01 / x1.18 [0.24]   x0.99 / x1.00 / x1.00 / x1.00 [0.21]
#    768 / 16  plain                  default = wide x1.01 / x1.00 / x1.04 / x1.02 [0.24]   x1.00 / x0.91 / x1.01 / x1.00 [0.15]   x0.99 / x1.00 / x1.01 / x1.05 [0.31]
#    768 / 16  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.02]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]
#    768 / 16  edge_hot               default        x0.99 / x1.00 / x1.01 / x1.00 [0.16]   x0.99 / x1.00 / x1.02 / x1.00 [0.17]   x1.00 / x1.00 / x1.01 / x1.00 [0.17]
#    768 / 16  frames_differ          default        x0.99 / x1.00 / x1.04 / x1.02 [0.22]   x1.01 / x0.99 / x1.01 / x1.00 [0.06]   x1.00 / x1.04 / x1.02 / x1.05 [0.29]
#    768 / 24  plain                  default = wide x1.00 / x1.00 / x1.01 / x1.00 [0.21]   x1.00 / x1.02 / x1.02 / x1.02 [0.22]   x0.99 / x1.00 / x1.01 / x1.06 [0.24]
#    768 / 24  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.01 / x1.00 / x1.02 [0.02]
#    768 / 24  edge_hot               default        x1.00 / x1.00 / x1.01 / x1.00 [0.18]   x1.00 / x1.01 / x1.00 / x1.02 [0.20]   x1.00 / x1.00 / x1.01 / x1.00 [0.17]
#    768 / 24  frames_differ          default        x1.01 / x1.00 / x1.03 / x1.00 [0.19]   x1.00 / x1.00 / x1.01 / x1.02 [0.18]   x1.00 / x1.00 / x1.01 / x1.17 [0.20]
#    384 / 16  plain                  default = wide x1.00 / x0.96 / x1.01 / x1.00 [0.18]   x0.99 / x1.00 / x1.01 / x1.12 [0.27]   x1.00 / x1.00 / x1.01 / x1.00 [0.06]
#    384 / 16  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.02]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]
#    384 / 16  edge_hot               default        x0.99 / x1.00 / x1.00 / x1.00 [0.21]   x1.00 / x1.03 / x1.00 / x1.03 [0.09]   x0.99 / x1.00 / x1.00 / x1.00 [0.17]
#    384 / 16  frames_differ          default        x1.00 / x0.96 / x1.00 / x1.10 [0.20]   x0.99 / x1.00 / x1.01 / x1.01 [0.22]   x1.00 / x1.00 / x1.01 / x1.05 [0.14]
#    384 / 24  plain                  default = wide x1.00 / x1.00 / x1.01 / x1.00 [0.14]   x1.00 / x1.00 / x1.01 / x1.19 [0.22]   x1.00 / x1.00 / x1.00 / x1.00 [0.21]
#    384 / 24  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.01]   x1.00 / x1.00 / x1.00 / x1.00 [0.01]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]
#    384 / 24  edge_hot               default        x1.00 / x1.00 / x1.00 / x1.00 [0.12]   x1.01 / x1.00 / x1.02 / x1.10 [0.16]   x1.01 / x1.01 / x1.02 / x1.16 [0.21]
#    384 / 24  frames_differ          default        x1.01 / x0.98 / x1.02 / x1.00 [0.14]   x1.00 / x1.00 / x1.01 / x1.19 [0.18]   x1.00 / x1.01 / x1.01 / x1.01 [0.15]
#    192 / 16  plain                  default = wide x1.00 / x1.00 / x1.01 / x1.00 [0.10]   x1.00 / x0.99 / x1.02 / x1.00 [0.05]   x1.00 / x0.95 / x1.02 / x1.00 [0.19]
#    192 / 16  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]   x1.00 / x1.00 / x1.00 / x1.00 [0.00]
#    192 / 16  edge_hot               default        x0.98 / x0.93 / x0.99 / x0.98 [0.15]   x1.00 / x1.00 / x1.01 / x1.00 [0.05]   x1.01 / x1.00 / x1.02 / x1.04 [0.16]
#    192 / 16  frames_differ          default        x1.01 / x1.00 / x1.01 / x1.00 [0.13]   x1.00 / x1.00 / x1.00 / x1.00 [0.03]   x1.00 / x0.91 / x1.02 / x1.00 [0.20]
#    192 / 24  plain                  default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.09]   x1.00 / x1.00 / x1.02 / x1.00 [0.14]   x1.00 / x1.00 / x1.01 / x1.00 [0.17]
#    192 / 24  one_token              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.04]   x1.00 / x1.00 / x1.00 / x1.00 [0.01]   x1.00 / x1.00 / x1.03 / x1.04 [0.03]
#    192 / 24  edge_hot               default        x0.99 / x0.99 / x1.00 / x1.00 [0.17]   x1.00 / x1.00 / x1.00 / x1.00 [0.14]   x1.00 / x0.93 / x1.01 / x1.00 [0.16]
#    192 / 24  frames_differ          default        x1.00 / x1.00 / x1.01 / x1.00 [0.11]   x1.00 / x1.00 / x1.00 / x1.00 [0.11]   x1.00 / x1.00 / x1.00 / x1.00 [0.11]
#   1024 / 24  B=1 plain              default = wide x1.00 / x0.98 / x1.00 / x0.98 [0.13]   x0.99 / x1.18 / x1.00 / x1.18 [0.25]   x1.00 / x1.00 / x1.00 / x1.00 [0.15]
#    768 / 24  B=1 plain              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.18]   x1.00 / x1.02 / x1.01 / x1.02 [0.18]   x0.99 / x1.00 / x1.01 / x1.00 [0.17]
#    384 / 24  B=1 plain              default = wide x1.01 / x1.00 / x1.01 / x1.00 [0.12]   x0.99 / x1.09 / x1.00 / x1.19 [0.24]   x0.99 / x1.00 / x1.00 / x1.00 [0.17]
#    192 / 24  B=1 plain              default = wide x1.00 / x1.00 / x1.00 / x1.00 [0.07]   x1.00 / x1.00 / x1.00 / x1.00 [0.07]   x0.99 / x0.97 / x1.00 / x1.00 [0.16]
#    768 / 24  sliced [0,1) + [1,3)   -              x0.99 / x1.00 / x1.00 / x1.00 [0.21]   x1.00 / x1.02 / x1.01 / x1.10 [0.19]   x1.01 / x1.00 / x1.02 / x1.03 [0.25]
#    768 / 24  sliced, frame 0        -              x0.98 / x0.97 / x0.98 / x0.97 [0.23]   x1.00 / x0.99 / x1.00 / x1.10 [0.21]   x1.00 / x0.92 / x1.01 / x0.99 [0.24]
#    768 / 24  sliced, frame 1        -              x1.00 / x1.00 / x1.00 / x1.00 [0.19]   x1.00 / x1.02 / x1.01 / x1.03 [0.18]   x1.02 / x0.99 / x1.02 / x1.03 [0.25]
#    768 / 24  sliced, frame 2        -              x1.00 / x1.00 / x1.00 / x1.00 [0.19]   x1.00 / x1.04 / x1.01 / x1.04 [0.19]   x1.00 / x1.00 / x1.01 / x1.00 [0.27]
# The kernels' error IS the oracle's: rel-L2 x0.98-1.02 in every case; kernel - oracle <= 0.06 of the oracle's error in one_token and
# 0.03-0.31 elsewhere (bf16 rounding-boundary flips through four layers; not asserted).  The worst 8 x 8 tile (printed, not asserted): x1.34.
FACTORS = {"score_map": 1.7, "size_map": 2.2, "offset_map": 1.8}


def errors(got, truth):
    d = np.asarray(got, np.float64) - truth
    return float(np.linalg.norm(d) / max(np.linalg.norm(truth), 1e-300)), float(np.abs(d).max())


def _tiles(a):
    """(B, ch, F, F) -> (B, ch, F / 8, F / 8, 64): the 8 x 8-pixel tiles of every channel."""
    B, ch, F, _ = a.shape
    return a.reshape(B, ch, F // 8, 8, F // 8, 8).transpose(0, 1, 2, 4, 3, 5).reshape(B, ch, F // 8, F // 8, 64)


def judge(name, kernel, truth, oracle, factor=None):
    """One map (B, ch, F, F): finite, and err(kernel) <= factor x err(oracle) + floor for rel-L2 and for max-abs, on the whole map and on
    every (frame, output channel) slot -- one wrong frame or channel cannot hide in the batch's norm.  The floor is FLOOR_ULPS f32 ulps at
    the truth's magnitude (the maps are stored as f32).  Reported, not asserted: the worst 8 x 8-pixel tile of a channel (64 values are too
    few for a stable ratio) and the kernel - oracle distance as a fraction of the oracle's error."""
    f = FACTORS[name] if factor is None else factor
    kernel, truth, oracle = (np.asarray(a, np.float64) for a in (kernel, truth, oracle))
    assert kernel.shape == truth.shape == oracle.shape and kernel.ndim == 4, (kernel.shape, truth.shape, oracle.shape)
    B, ch = truth.shape[:2]
    finite = bool(np.isfinite(kernel).all())
    k_rel, k_abs = errors(kernel, truth)
    o_rel, o_abs = errors(oracle, truth)
    b_rel = f * o_rel + FLOOR_ULPS * EPS32
    b_abs = f * o_abs + FLOOR_ULPS * EPS32 * float(np.abs(truth).max())
    dk, do, tr = ((a.reshape(B, ch, -1)) for a in (kernel - truth, oracle - truth, truth))
    tn = np.maximum(np.linalg.norm(tr, axis=-1), 1e-300)
    sk_rel, so_rel = np.linalg.norm(dk, axis=-1) / tn, np.linalg.norm(do, axis=-1) / tn
    sk_abs, so_abs = np.abs(dk).max(-1), np.abs(do).max(-1)
    with np.errstate(invalid="ignore"):
        ex_rel = np.where(np.isfinite(sk_rel), sk_rel / (f * so_rel + FLOOR_ULPS * EPS32), np.inf)
        ex_abs = np.where(np.isfinite(sk_abs), sk_abs / (f * so_abs + FLOOR_ULPS * EPS32 * np.abs(tr).max(-1)), np.inf)
        ra_rel = np.where(np.isfinite(sk_rel), sk_rel / np.maximum(so_rel, 1e-300), np.inf)
        ra_abs = np.where(np.isfinite(sk_abs), sk_abs / np.maximum(so_abs, 1e-300), np.inf)
    excess = np.maximum(ex_rel, ex_abs)                                   # > 1: the slot is over its bound
    worst = np.unravel_index(int(np.argmax(excess)), excess.shape)
    tile_ratio = float("nan")
    if truth.shape[-1] % 8 == 0 and finite:
        tk, to = np.linalg.norm(_tiles(kernel - truth), axis=-1), np.linalg.norm(_tiles(oracle - truth), axis=-1)
        tile_ratio = float((tk / np.maximum(to, 1e-300)).max())
    ko = errors(kernel, oracle)[0] * float(np.linalg.norm(oracle) / max(np.linalg.norm(truth), 1e-300))
    return {"stage": name, "kernel_rel": k_rel, "kernel_abs": k_abs, "oracle_rel": o_rel, "oracle_abs": o_abs, "bound_rel": b_rel,
            "bound_abs": b_abs, "ratio_rel": k_rel / max(o_rel, 1e-300), "ratio_abs": k_abs / max(o_abs, 1e-300),
            "slot": tuple(int(i) for i in worst), "slot_ratio_rel": float(ra_rel.max()), "slot_ratio_abs": float(ra_abs.max()),
            "slot_excess": float(excess.max()), "tile_ratio": tile_ratio, "ko_rel": ko, "ko_frac": ko / max(o_rel, 1e-300), "finite": finite,
            "worst": float(max(k_rel / max(o_rel, 1e-300), k_abs / max(o_abs, 1e-300), ra_rel.max(), ra_abs.max())),
            "ok": finite and k_rel <= b_rel and k_abs <= b_abs and float(excess.max()) <= 1.0}


def judge_all(kernel, truth, oracle, factor=None):
    """``judge`` for the three maps: [record per map]."""
    return [judge(k, kernel[k], truth[k], oracle[k], factor) for k in MAPS]


def fmt(r):
    return (f"{r['stage']:>10}: rel {r['kernel_rel']:.2e} (oracle {r['oracle_rel']:.2e}, x{r['ratio_rel']:.2f}, bound {r['bound_rel']:.2e})"
            f"  abs {r['kernel_abs']:.2e} (oracle {r['oracle_abs']:.2e}, x{r['ratio_abs']:.2f}, bound {r['bound_abs']:.2e})"
            f"  worst slot (frame, channel) {r['slot']} rel x{r['slot_ratio_rel']:.2f} abs x{r['slot_ratio_abs']:.2f}"
            f"  [8 x 8 tile x{r['tile_ratio']:.2f}  kernel-oracle {r['ko_rel']:.2e} = {r['ko_frac']:.2f} of the oracle's]"
            + ("" if r["ok"] else "  OVER"))
