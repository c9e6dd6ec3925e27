"""CPU: the feature regimes of tests/bf16_head_budget.py have the properties they are built for, the helper's truth is the pinned torch
oracle's head, the bf16 oracle's error sits in a stated band, and the budget has teeth -- every emulated head defect leaves it in every
regime listed for it, with FACTORS as committed.  fp64 numpy + bf16 rounding by torch; no GPU.

Geometries: widths 1024 / 768 / 384 / 192 at F = 16 (B = 2) and F = 24 (B = 3); one_token always nine frames, run as launches of B.

The oracle's error against the truth, plain regime, rel-L2 / max-abs (seed 26), per width at F = 16 | F = 24:
             score_map                              size_map                               offset_map
  1024   5.4e-3 / 9.3e-3 | 3.5e-3 / 1.4e-2     2.1e-3 / 6.9e-3 | 2.3e-3 / 9.1e-3     8.1e-3 / 2.0e-2 | 5.4e-3 / 1.8e-2
   768   4.1e-3 / 1.2e-2 | 5.9e-3 / 1.2e-2     3.8e-3 / 8.9e-3 | 4.3e-3 / 6.6e-3     5.2e-3 / 2.2e-2 | 4.6e-3 / 2.5e-2
   384   5.7e-3 / 1.3e-2 | 4.5e-3 / 1.1e-2     4.5e-3 / 6.8e-3 | 3.5e-3 / 1.1e-2     5.7e-3 / 1.5e-2 | 3.9e-3 / 1.9e-2
   192   3.1e-3 / 5.3e-3 | 2.5e-3 / 1.3e-2     3.4e-3 / 9.6e-3 | 2.3e-3 / 7.2e-3     4.6e-3 / 2.4e-2 | 4.6e-3 / 2.0e-2
``BANDS`` is the smallest of these x 0.6 to the largest x 1.4, per map.  one_token's error is smaller (rel-L2 4e-4 .. 3.4e-3: most of a map
is the constant the biases alone give), edge_hot's and frames_differ's rel-L2 are plain's within 30 %.

Share of the truth's score / size values on the sigmoid clamp: plain <= 0.02 %, one_token 0, edge_hot <= 0.98 % (384 / 16; else <= 0.13 %),
frames_differ <= 0.29 % (192 / 24).

Defects (``head(defect=)``, emulated on the bf16 oracle): the worst of rel-L2, max-abs and the (frame, channel) slots' two ratios, error /
the oracle's error, over the maps a defect touches; smallest .. largest over the eight geometries and the four regimes:

  tower_w2   conv2 weights of the offset and size towers exchanged (gW)      x173 .. x661    score_map untouched (x1.00)
  bias0_l2   conv2 of every tower takes tower 0's bias (gBias)               x33 .. x595     plain / edge_hot / frames_differ x33-68, one_token >= x151
  norelu4    no ReLU after conv4                                             x129 .. x1466
  taps_T     conv1's taps transposed                                         x154 .. x286
  edge_l1    layer 1 reads a replicated border instead of zero               x48 .. x245
  edge_l2    layer 2                                                         x44 .. x218
  edge_l3    layer 3                                                         x49 .. x200
  edge_l4    layer 4                                                         x68 .. x325
  w5swap     conv5's two offset rows exchanged                               x217 .. x1174   offset_map only
  pad32      the last 8 of conv4's 32 columns never written                  x83 .. x619
  straddle   conv4's rows past a frame boundary inside a 256-row tile        x155 .. x583 at F = 24 (B = 3); x1.00 at F = 16
  droptail   conv4's last, partial 256-row tile not written                  x157 .. x542 at F = 24;         x1.00 at F = 16

The smallest ratio a defect reaches in a catching regime is x32.9 (bias0_l2, frames_differ, width 192 at F = 16, size_map); a factor must
stay at or below a third of it, 10.9, which ``test_every_defect_leaves_the_budget`` asserts for every (defect, regime, geometry) it runs.
It runs the geometries 768 / 16, 192 / 24, 1024 / 24 and 384 / 16 (each width once, each map size twice); the figures above are from a run
of all eight.
"""
import numpy as np
import pytest

import bf16_head_budget as hb

WIDTHS = (1024, 768, 384, 192)
DEFECT_GEOMS = ((768, 16), (192, 24), (1024, 24), (384, 16))
BANDS = {         # map -> ((rel-L2 lo, hi), (max-abs lo, hi)) of the oracle's error in `plain`: measured smallest x 0.6 .. largest x 1.4
    "score_map": ((1.5e-3, 8.2e-3), (3.2e-3, 2.0e-2)),
    "size_map": ((1.2e-3, 6.3e-3), (4.0e-3, 1.6e-2)),
    "offset_map": ((2.4e-3, 1.14e-2), (9.0e-3, 3.6e-2)),
}
_CASES = {}


def _case(C, F, name):
    """Per (width, map size, regime), once: the state dict, features, fp64 truth, bf16 oracle and the oracle's tower layers (for the
    defects).  One (width, map size) is kept at a time: the cases come geometry by geometry."""
    if (C, F, name) not in _CASES:
        for key in [k for k in _CASES if k[:2] != (C, F)]:
            del _CASES[key]
        sd = hb.state(C, F)
        B = 9 if name == "one_token" else hb.GEOMS[F][2]
        X = hb.regime(name, B, F, C)
        memo = {}
        _CASES[(C, F, name)] = {"sd": sd, "X": X, "truth": hb.head(sd, X, "truth"), "oracle": hb.head(sd, X, "bf16", memo=memo), "memo": memo}
    return _CASES[(C, F, name)]


_GEOMS = [(C, F) for C in WIDTHS for F in (16, 24)]


@pytest.mark.parametrize("C,F,name", [pytest.param(C, F, n, id=f"{C}-{F}-{n}") for C, F in _GEOMS for n in hb.REGIMES])
def test_regime_has_its_property(C, F, name):
    c = _case(C, F, name)
    X, truth, oracle = c["X"], c["truth"], c["oracle"]
    B = X.shape[0]
    assert X.dtype == np.float32 and X.shape == (9 if name == "one_token" else hb.GEOMS[F][2], F * F, C)
    for k, ch in zip(hb.MAPS, (1, 2, 2)):
        assert truth[k].shape == oracle[k].shape == (B, ch, F, F) and truth[k].dtype == np.float64
    share = hb.clamp_share(truth)
    print(C, F, name, "clamp share", share)
    assert share <= 0.01, share
    if name == "one_token":
        zero = hb.head(c["sd"], np.zeros((1, F * F, C), np.float32), "truth")
        for i, (y, x) in enumerate(hb.pixels(F)):
            assert np.count_nonzero(X[i]) == C and np.count_nonzero(X[i, y * F + x]) == C
            win = np.zeros((F, F), bool)
            win[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5] = True
            for k in hb.MAPS:
                d = np.abs(truth[k][i] - zero[k][0]).max(0)
                assert d[~win].max() <= 1e-12, (k, i, d[~win].max())          # nothing outside the receptive field
            d = np.abs(truth["offset_map"][i] - zero["offset_map"][0]).max(0)          # (no sigmoid: nothing flattens a change)
            ys, xs = np.nonzero(d > 1e-9)
            assert (ys.min(), ys.max(), xs.min(), xs.max()) == (max(y - 4, 0), min(y + 4, F - 1), max(x - 4, 0), min(x + 4, F - 1)), (i, y, x)
            assert (d[win] > 1e-9).mean() >= 0.9, (i, (d[win] > 1e-9).mean())
    elif name == "edge_hot":
        e = (X.astype(np.float64) ** 2).reshape(B, F, F, C).sum((0, 3))
        assert e[hb.ring(F)].sum() / e.sum() >= 0.60
    elif name == "frames_differ":
        for k in hb.MAPS:
            err = oracle[k] - truth[k]
            for a in range(B):
                for b in range(a + 1, B):
                    d = truth[k][a] - truth[k][b]
                    assert np.linalg.norm(d) >= 10.0 * max(np.linalg.norm(err[a]), np.linalg.norm(err[b])), (k, a, b)
                    assert np.abs(d).max() >= 10.0 * max(np.abs(err[a]).max(), np.abs(err[b]).max()), (k, a, b)


@pytest.mark.parametrize("C,F", [pytest.param(C, F, id=f"{C}-{F}") for C, F in _GEOMS])
def test_oracle_error_band(C, F):
    """The bf16 oracle's own error against the truth, plain regime, inside BANDS per map; the oracle judged as a kernel sits at x1.00."""
    c = _case(C, F, "plain")
    for r in hb.judge_all(c["oracle"], c["truth"], c["oracle"]):
        print(C, F, hb.fmt(r))
        (rlo, rhi), (alo, ahi) = BANDS[r["stage"]]
        assert rlo <= r["oracle_rel"] <= rhi and alo <= r["oracle_abs"] <= ahi, r
        assert r["ok"] and r["worst"] == 1.0 and r["ko_rel"] == 0.0


def _defect(C, F, name, d):
    c = _case(C, F, name)
    got = hb.head(c["sd"], c["X"], "bf16", defect=d, batch=hb.GEOMS[F][2], memo=c["memo"])
    return hb.judge_all(got, c["truth"], c["oracle"])


@pytest.mark.parametrize("C,F,d", [pytest.param(C, F, d, id=f"{C}-{F}-{d}") for C, F in DEFECT_GEOMS for d in hb.DEFECTS])
def test_every_defect_leaves_the_budget(C, F, d):
    """A defect is over the budget in exactly its CATCHES regimes, there by at least 3 x the map's factor in one figure of one map; in the
    others (the tile defects at F = 16) it is invisible: under the budget, within 10 % of the oracle's error."""
    for name in hb.REGIMES:
        rs = _defect(C, F, name, d)
        print(C, F, d, name, " ".join(f"{r['stage']} x{r['worst']:.1f}" for r in rs))
        if name in hb.CATCHES[d][F]:
            assert not all(r["ok"] for r in rs), (name, rs)
            assert all(r["finite"] for r in rs)
            assert any(r["worst"] >= 3.0 * hb.FACTORS[r["stage"]] for r in rs), (name, rs)
        else:
            assert all(r["ok"] and r["worst"] < 1.1 for r in rs), (name, rs)


def test_factors_are_capped():
    """A third of the smallest ratio a defect reaches in a catching regime (x32.9, the docstring's table)."""
    assert all(f <= 32.9 / 3.0 for f in hb.FACTORS.values()) and set(hb.FACTORS) == set(hb.MAPS)


@pytest.mark.parametrize("C", WIDTHS)
def test_truth_is_the_pinned_torch_oracles_head(C):
    """The helper's fp64 truth against oracle/vitb_oracle_torch.py's head (fp32) on one synthetic state dict per width: 1e-5 max-abs on the
    three maps.  The oracle runs in fp32, so this holds the layout (NCHW maps, tap order, BN, tower and channel order), not the precision."""
    import torch
    from oracle import vitb_oracle_torch as vo
    F = 16
    c = _case(C, F, "plain")
    m = vo.build_from_state(c["sd"], heads=hb.WIDTHS[C].heads)
    B = c["X"].shape[0]
    with torch.no_grad():
        f = torch.from_numpy(c["X"]).transpose(1, 2).reshape(B, C, F, F).contiguous()
        score, _, size, offset = m.box_head(f)
    for k, got in zip(hb.MAPS, (score, size, offset)):
        err = float(np.abs(got.numpy().astype(np.float64) - c["truth"][k]).max())
        print(C, k, err)
        assert got.shape == c["truth"][k].shape and err <= 1e-5, (k, err)
