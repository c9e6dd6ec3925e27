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
  head_shift       q, k of head h with v of head    plain x279 (x278) at 320, x316 (x180) at 720
                   (h + 1) mod heads

The smallest ratio a defect reaches in a catching regime is x26 (swap4_v, peaked, max-abs); FACTORS["attn"] must stay at or below a third
of it, which ``test_every_defect_leaves_the_budget`` asserts for every (defect, regime) pair.

Widths 1024 / 384 / 192 (``bb.WIDTHS``, regimes at the width's amplitudes ``bb.AMPS``, whose comment holds the measured ramp and hot-key
properties): the same property and defect tests with the same assertions, ids led by the width; the ViT-Base cases keep their ids and
print the numbers above.  peaked spread 112.9 / 122.8, 113.5 / 119.7, 109.0 / 117.3 (320 / 720); below_zero largest logit -29.4 / -29.1,
-32.2 / -30.3, -26.7 / -31.1.  Defects there, rel-L2 (max-abs) at 1024 | 384 | 192:

  no_O_rescale     plain 320      x179 (x481) | x179 (x459) | x197 (x527)        peaked 320    x81 (x32) | x79 (x39) | x89 (x45)
                   ramp_up 320    x375 (x544) | x309 (x351) | x229 (x221)        ramp_up 720   x1212 | x894 | x1003
  no_l_rescale     ramp_up 320    x109 (x82) | x106 (x52) | x76 (x46)            ramp_up 720   x251 | x232 | x225
  lane_group_max   last_keys and first_keys, both geometries: inf / NaN at every width
  pad_leak         below_zero 720 x98 (x60) | x98 (x62) | x111 (x51)
  pad_v_nan        NaN in plain, peaked, below_zero at every width
  drop_last16      last_keys 320  x132 (x59) | x75 (x40) | x103 (x56)            720           x111 | x101 | x163
  swap4_v          plain 320      x198 (x268) | x200 (x149) | x209 (x211)        peaked 320    x97 (x22) | x95 (x27) | x104 (x36)
                   plain 720      x194 | x199 | x209
  no_log2e         plain 320      x69 (x92) | x69 (x77) | x70 (x107)             plain 720     x69 (x120) | x70 (x101) | x70 (x84)
  head_shift       plain 320      x272 (x228) | x283 (x186) | x291 (x220)        plain 720     x307 | x312 | x336

The smallest of max(rel-L2, max-abs) over every (defect, regime, width) there is x74.7 (drop_last16, last_keys, 320 tokens, width 384);
the smallest single figure x22 (swap4_v, peaked, max-abs, width 1024, whose rel-L2 is x97) -- both >= 3 x 1.65 = 4.95.
"""
import numpy as np
import pytest

import bf16_budget as bb
from vitb_u8_fold import rel_c

_CASES = {}


def _case(L, name, C=768):
    """Per (width, geometry, regime), once: fp64 truth of attention alone, the bf16 q / k / v and the oracle (its two forms on demand).
    One width is kept at a time (the cases come width by width), so what stays resident is what the ViT-Base cases alone kept."""
    if (C, L, name) not in _CASES:
        for key in [k for k in _CASES if k[0] != C]:
            del _CASES[key]
        w = bb.WIDTHS[C]
        sd, X = bb.regime(name, L, w=w)
        truth = bb.attention(*bb.qkv(sd, X, 0, "truth", w=w))
        _CASES[(C, L, name)] = {"truth": truth, "qkv": bb.qkv(sd, X, 0, "bf16", w=w), "at": X.astype(np.float64) + truth}
    return _CASES[(C, L, name)]


def _oracle(c, form):
    if form not in c:
        c[form] = bb.attention(*c["qkv"], "bf16", chunk=bb.KC if form == "stream" else None)
    return c[form]


NEW_WIDTHS = (1024, 384, 192)


def _ids(cases):
    """pytest.param per (C, ...) case: the ViT-Base cases keep the ids they had before the width was a parameter, the others lead with it."""
    return [pytest.param(*c, id="-".join(str(v) for v in (c[1:] if c[0] == 768 else c))) for c in cases]


@pytest.mark.parametrize("C,name,L", _ids([(C, n, L) for C in (768,) + NEW_WIDTHS for L in (320, 720) for n in bb.REGIMES]))
def test_regime_has_its_property(C, name, L):
    w = bb.WIDTHS[C]
    sd, X = bb.regime(name, L, w=w)
    assert X.shape == (2, L, C) and X.dtype == np.float32
    p = bb.properties(bb.logits(sd, X, w=w))
    print(C, L, name, {k: round(v, 3) for k, v in p.items()})
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


@pytest.mark.parametrize("C,L", _ids([(768, 320), (768, 720)] + [(C, 320) for C in NEW_WIDTHS]))
def test_oracle_one_block_error_is_the_devices(C, L):
    """One whole block (real proj / MLP weights, plain regime) of the bf16 oracle against fp64, on the rows' centred norm: inside
    [1.0e-3, 1.3e-3] at both geometries (1.17e-3 / 1.12e-3) -- the device's recorded 1.16e-3 / 1.14e-3 (NOTES.md): the oracle models
    the hardware.  Both forms of the oracle's softmax (whole row / 64-key chunks) agree on it.
    At widths 1024 / 384 / 192 and 320 tokens: inside [0.8e-3, 1.5e-3]; measured 1.18e-3 / 1.18e-3 / 1.19e-3 in either softmax form
    (1.182e-3 / 1.176e-3 / 1.188e-3 whole row, 1.181e-3 / 1.174e-3 / 1.191e-3 chunked).  The device's recorded figures after one
    block of the reference fixtures at widths 384 / 192 are 1.19e-3 / 1.18e-3 (tests/test_gpu_vit_small.py)."""
    w = bb.WIDTHS[C]
    lo, hi = (1.0e-3, 1.3e-3) if C == 768 else (0.8e-3, 1.5e-3)
    sd, X = bb.regime("plain", L, w=w)
    truth = bb.run(sd, X, 1, "truth", w=w)[0][0]
    for chunk in (None, bb.KC):
        e = rel_c(bb.run(sd, X, 1, "bf16", chunk=chunk, w=w)[0][0], truth)
        print(C, L, chunk, e)
        assert lo <= e <= hi, (C, L, chunk, e)


@pytest.mark.parametrize("L,name", [(320, "plain"), (320, "peaked"), (320, "ramp_up"), (720, "plain"), (720, "last_keys"), (720, "below_zero")])
def test_the_two_oracle_forms_hold_each_others_budget(L, name):
    """The streaming form (P rounded against the running maximum, l and O rescaled) judged as a kernel against the whole-row form: two
    correct bf16 attentions sit inside the budget of one another, in all three figures."""
    c = _case(L, name)
    r = bb.judge("attn", _oracle(c, "stream"), c["truth"], _oracle(c, "plain"), at=c["at"])
    print(bb.fmt(r))
    assert r["ok"] and r["ratio_rel"] < 1.1 and r["slot_ratio"] < 1.3, r


def _defect(d, L, name, C=768):
    c = _case(L, name, C)
    group = bb.hot_group(L) if name == "first_keys" else 0
    got = bb.attention(*c["qkv"], "bf16", defect=d, group=group)
    return bb.judge("attn", got, c["truth"], _oracle(c, "stream" if d in bb.STREAM_DEFECTS else "plain"), at=c["at"], w=bb.WIDTHS[C])


@pytest.mark.parametrize("C,d,L,name", _ids([(C, d, L, n) for C in (768,) + NEW_WIDTHS for d in bb.DEFECTS
                                             for L, names in bb.CATCHES[d].items() for n in names]))
def test_every_defect_leaves_the_budget(C, d, L, name):
    """In its catching regime a defect is over the bound, and by at least 3 x FACTORS in one of the three figures (or not finite): the
    factor is at most a third of what the defect reaches -- at every width, judged with the judge the GPU modules use."""
    r = _defect(d, L, name, C)
    print(C, d, bb.fmt(r))
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
