"""CPU: the softmax regimes of tests/bf16_budget.py have the properties they are built for, the bf16 oracle models the device, and the
budget has teeth -- every emulated attention defect leaves it in the regime named below.  fp64 numpy + bf16 rounding by torch; no GPU.

Regime properties (B = 2, seed 26; measured at 320 / 720 tokens):

  peaked       largest per-row logit spread >= 100                                          112.5 / 127.4 (mean top probability 0.83 / 0.81)
  ramp_up      the 64-key running maximum moves at EVERY boundary for >= 90 % of rows (320)   1.00;   on average >= 9 of 11 (720): 10.3
  ramp_down    it never moves after chunk 0 for >= 70 %                                       1.00 / 0.94
  last_keys    argmax in the last 16 keys for >= 95 %; the eight hot logits clear every
               other key of their row by more than ln(f32 max) = 88.7                        1.00 / 1.00; smallest gap 98.7 / 99.4
  first_keys   the same with keys 0..7 hot: argmax in the first 16, the maximum never moves   1.00 / 1.00; smallest gap 97.6 / 99.2
  below_zero   every real logit <= -20                                                       fraction 1.0; largest logit -30.0 / -29.1
  plain, common_mode: none (the running maximum moves 1.27 times in 4 boundaries / 2.05 in 11, never for 20 % / 9 % of the rows)

Defects (tests/bf16_budget.py ``attention(defect=)``): error / the oracle's error, rel-L2 (max-abs), in the regimes that must catch them
(``CATCHES``) and, in brackets, in regimes that cannot:

  no_O_rescale     O not rescaled by alpha          plain x178 (x517), peaked x80 (x38), ramp_up x301 (x271) at 320; ramp_up x1020 at 720
                                                    [ramp_down x1.07, first_keys x1.00: the maximum never moves]
  no_l_rescale     lsum not rescaled                ramp_up x99 (x53) at 320, x255 (x168) at 720   [first_keys x1.00]
  lane_group_max   the row maximum taken over the   last_keys (group 0) and first_keys (the group that holds last_keys' hot keys): inf / NaN, so
                   keys of ONE lane group           every group is caught by one of the two at both geometries.
                                                    [peaked x1.00 -- a FINDING against the issue's expectation: a spread of 112 is max - min of
                                                    a row; overflow needs the row maximum to clear the best of a QUARTER of the keys by 88.7,
                                                    and among 80 random keys one is always within a few units of it.  Hence the two hot-key regimes]
  pad_leak         16 zero-K pad keys with the      below_zero x105 (x53)
                   neighbour frame's V at 720       [plain x4.2 (x1.4): caught by a factor below 4.2 only; peaked, ramps, last_keys x1.00]
  pad_v_nan        score masked, V^T column NaN     NaN in every regime (0 x NaN): plain, peaked, below_zero are run
  drop_last16      the last 16 real keys dropped    last_keys x125 (x71) at 320, x105 (x57) at 720   [ramp_down, first_keys x1.00]
  swap4_v          keys j, j ^ 4 exchanged on the   plain x200 (x194), peaked x97 (x26) at 320; plain x197 at 720
                   V^T side only
  no_log2e         exp2 without the log2 e factor   plain x69 (x113) at 320, x70 (x87) at 720   [peaked only x8.5 (x3.3)]

The smallest ratio a defect reaches in a catching regime is x26 (swap4_v, peaked, max-abs); FACTORS["attn"] must stay at or below a third
of it, which ``test_every_defect_leaves_the_budget`` asserts for every (defect, regime) pair.
"""
import numpy as np
import pytest

import bf16_budget as bb
from vitb_u8_fold import rel_c

_CASES = {}


def _case(L, name):
    """Per (geometry, regime), once: fp64 truth of attention alone, the bf16 q / k / v and both forms of the oracle."""
    if (L, name) not in _CASES:
        sd, X = bb.regime(name, L)
        truth = bb.attention(*bb.qkv(sd, X, 0, "truth"))
        q, k, v = bb.qkv(sd, X, 0, "bf16")
        _CASES[(L, name)] = {"truth": truth, "qkv": (q, k, v), "at": X.astype(np.float64) + truth,
                             "plain": bb.attention(q, k, v, "bf16"), "stream": bb.attention(q, k, v, "bf16", chunk=bb.KC)}
    return _CASES[(L, name)]


@pytest.mark.parametrize("L", [320, 720])
@pytest.mark.parametrize("name", bb.REGIMES)
def test_regime_has_its_property(name, L):
    sd, X = bb.regime(name, L)
    assert X.shape == (2, L, 768) and X.dtype == np.float32
    p = bb.properties(bb.logits(sd, X))
    print(L, name, {k: round(v, 3) for k, v in p.items()})
    assert p["boundaries"] == {320: 4, 720: 11}[L]
    if name == "peaked":
        assert p["spread"] >= 100.0
    elif name == "ramp_up":
        assert p["moves_all"] >= 0.90 if L == 320 else p["moves_mean"] >= 9.0
    elif name == "ramp_down":
        assert p["moves_none"] >= 0.70
    elif name == "last_keys":
        assert p["argmax_last16"] >= 0.95 and p["hot_gap"] > 88.73
    elif name == "first_keys":
        assert p["argmax_first16"] >= 0.95 and p["moves_none"] == 1.0 and p["hot_gap"] > 88.73
    elif name == "below_zero":
        assert p["below_m20"] == 1.0 and p["max_logit"] <= -20.0


@pytest.mark.parametrize("L", [320, 720])
def test_oracle_one_block_error_is_the_devices(L):
    """One whole block (real proj / MLP weights, plain regime) of the bf16 oracle against fp64, on the rows' centred norm: inside
    [1.0e-3, 1.3e-3] at both geometries (1.17e-3 / 1.12e-3) -- the device's recorded 1.16e-3 / 1.14e-3 (NOTES.md): the oracle models
    the hardware.  Both forms of the oracle's softmax (whole row / 64-key chunks) agree on it."""
    sd, X = bb.regime("plain", L)
    truth = bb.run(sd, X, 1, "truth")[0][0]
    for chunk in (None, bb.KC):
        e = rel_c(bb.run(sd, X, 1, "bf16", chunk=chunk)[0][0], truth)
        print(L, chunk, e)
        assert 1.0e-3 <= e <= 1.3e-3, (L, chunk, e)


@pytest.mark.parametrize("L,name", [(320, "plain"), (320, "peaked"), (320, "ramp_up"), (720, "plain"), (720, "last_keys"), (720, "below_zero")])
def test_the_two_oracle_forms_hold_each_others_budget(L, name):
    """The streaming form (P rounded against the running maximum, l and O rescaled) judged as a kernel against the whole-row form: two
    correct bf16 attentions sit inside the budget of one another, in all three figures."""
    c = _case(L, name)
    r = bb.judge("attn", c["stream"], c["truth"], c["plain"], at=c["at"])
    print(bb.fmt(r))
    assert r["ok"] and r["ratio_rel"] < 1.1 and r["slot_ratio"] < 1.3, r


def _defect(d, L, name):
    c = _case(L, name)
    group = bb.hot_group(L) if name == "first_keys" else 0
    got = bb.attention(*c["qkv"], "bf16", defect=d, group=group)
    return bb.judge("attn", got, c["truth"], c["stream" if d in bb.STREAM_DEFECTS else "plain"], at=c["at"])


@pytest.mark.parametrize("d,L,name", [(d, L, n) for d in bb.DEFECTS for L, names in bb.CATCHES[d].items() for n in names])
def test_every_defect_leaves_the_budget(d, L, name):
    """In its catching regime a defect is over the bound, and by at least 3 x FACTORS in one of the three figures (or not finite): the
    factor is at most a third of what the defect reaches."""
    r = _defect(d, L, name)
    print(d, bb.fmt(r))
    assert not r["ok"], r
    if d in ("lane_group_max", "pad_v_nan"):
        assert not r["finite"]
    else:
        assert r["finite"] and max(r["ratio_rel"], r["ratio_abs"]) >= 3.0 * bb.FACTORS["attn"], r


@pytest.mark.parametrize("d,L,name", [("lane_group_max", 320, "peaked"), ("pad_leak", 720, "peaked"), ("no_O_rescale", 320, "ramp_down"),
                                      ("drop_last16", 320, "ramp_down")])
def test_regimes_that_cannot_see_a_defect(d, L, name):
    """Why the other regimes exist: a quarter-row maximum in `peaked`, a leaked pad key in `peaked`, a missing rescale or sixteen missing
    keys in `ramp_down` change the result by less than the oracle's own error -- rel-L2 within 10 % of the oracle's."""
    r = _defect(d, L, name)
    print(d, bb.fmt(r))
    assert r["finite"] and r["ratio_rel"] < 1.1, r
